// Marginal state covariance (okvis_ba_state_covariance, DESIGN.md "State covariance"): selected rows / columns of the inverse of
// the undamped reduced system S0 that solve_kernel(final_only = 2) exports.  One workgroup per window, one matrix row per work-item:
//   1. Jacobi scaling by powers of two, S^ = diag(d) S0 diag(d) with d_i = 1 / sqrt(S0_ii) rounded to a power of two (diagonal in
//      [0.5, 2); the scaling and its undoing are exact, so S^ is known to the last bit), lower triangle to LDS, row-packed;
//   2. left-looking Cholesky in place, then the factor is inverted in place (M = L^-1), column by column from the last: both are
//      chains of D dependent columns with two barriers each, every dot product in index order;
//   3. the selected unit vectors, 15 columns at a time: X = M^T (M E) — products without a dependent chain — then two steps of
//      iterative refinement, X += M^T M (E - S^ X), the residual accumulated with error-free products and sums (twice the working
//      precision, Ogita / Rump / Oishi's Dot2).  The undamped system has a condition of 1e8 ... 1e11 after scaling: plain fp64
//      leaves cond x eps = 1e-8 ... 1e-5 in the result, as any fp64 host inverse does; the refinement takes that to the rounding
//      of the result itself;
//   4. Sigma_K = diag(d_K) X_K diag(d_K): the entry of the lower triangle (in ascending row order) is computed, the upper mirrored.
// The body is the device function cov_solve, shared by cov_kernel (a list of rows: okvis_ba_state_covariance) and cov_pose_kernel
// (all pose-type rows, written to HBM: stage one of okvis_ba_landmark_covariance and okvis_ba_predicted_measurement, ba_lmcov.hpp,
// ba_predcov.hpp).  The file also holds cov_dot2_step, the error-free accumulation step of every refinement in the three entries,
// and cov_keep_kernel, which keeps and restores what the assembly launches overwrite.
// Route chosen among the two of the issue: unit vectors, not "K last and the trailing Schur complement".  The trailing block needs
// no second array but cannot be refined (its error is in the complement, not in the small inverse); the unit vectors need D x 15
// doubles next to the packed triangle (119 + 20 KB at D = 174) and give every column the same arithmetic whatever else is
// selected, so a result does not depend on the order of the list.
// fp64 throughout, no atomics on doubles, every sum in a fixed order: a window's result has the same bits alone or in any batch.
// The matrix core is not used: the kernel's time is the two chains of dependent columns (barriers and LDS latency, D^3 / 3 = 1.8
// Mflop each at the limit), not arithmetic (profiles/cov_notes.md).
#pragma once
#include "ba_types.hpp"

namespace ba {

constexpr int COV_THREADS = 256;
constexpr int COV_MAX_DIM = 30;   // OKVIS_BA_COV_MAX_DIM
constexpr int COV_KC = 15;        // columns solved together
constexpr int COV_REFINE = 2;     // refinement steps
static_assert(MAX_D_LDS <= COV_THREADS, "one matrix row per work-item");

struct CovArgs {
  const double* S;   // [D][D] the exported system, full symmetric
  double* out;       // cov [k][k] (rows ascending) | min_pivot | info (int)
  int D, k;
  int rows[COV_MAX_DIM];   // the selected reduced rows, ascending
};

__host__ __device__ constexpr size_t cov_lds_bytes(int D) { return 8 * ((size_t)D * (D + 1) / 2 + (size_t)D * COV_KC + D); }
__host__ __device__ constexpr size_t cov_out_doubles(int k) { return (size_t)k * k + 2; }

// One step of a dot product in twice the working precision (Ogita / Rump / Oishi's Dot2): hi + lo += a b, the product and the sum
// as error-free transformations.  Every refinement of the covariance entries forms its residual with it: cov_solve below, the
// 3 x 3 steps of ba_lmcov.hpp and ba_predcov.hpp.
__device__ __forceinline__ void cov_dot2_step(double a, double b, double& hi, double& lo) {
#pragma clang fp contract(off)   // (the sums below are error-free only as written)
  const double p = a * b;
  const double pe = __builtin_fma(a, b, -p);
  const double sum = hi + p;
  const double bb = sum - hi;
  const double se = (hi - (sum - bb)) + (p - bb);
  hi = sum;
  lo += pe + se;
}

// Which reduced rows are selected: a list (cov_kernel) or the leading k (cov_pose_kernel).  Ascending either way.
struct CovRowList {
  const int* r;
  __device__ __forceinline__ int operator()(int q) const { return r[q]; }
};
struct CovRowLeading {
  __device__ __forceinline__ int operator()(int q) const { return q; }
};

// The whole of a window's work, shared by the two kernels below: columns rows(0 .. k-1) of S^-1, the k x k result to `out`
// (row-major, bitwise symmetric), min_pivot and info to tail[0], tail[1].  A column's arithmetic does not depend on what else is
// selected: entry (a, b) has the same bits in either kernel.
template <class Rows>
__device__ __forceinline__ void cov_solve(const double* S, double* out, double* tail, int D, int k, const Rows rows) {
  extern __shared__ __attribute__((aligned(16))) double cov_smem[];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  const int nL = D * (D + 1) / 2;
  double* L = cov_smem;            // packed lower triangle, row i at i (i + 1) / 2: S^, then its factor, then the factor's inverse
  double* Wm = L + nL;             // [D][COV_KC]: right-hand sides and intermediate vectors
  double* sd = Wm + D * COV_KC;    // the scaling d
  const double nan = __builtin_nan("");
  const bool row = tid < D;        // this work-item has a row
  const int ri = row ? tid : 0;
  double* const Li = L + ri * (ri + 1) / 2;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  bool bad = false;
  if (row) {
    const double v = S[(size_t)tid * D + tid];
    if (!(v > 0.0) || !(v < __builtin_inf())) {
      bad = true;
      sd[tid] = 1.0;
    } else {
      int e;
      (void)frexp(v, &e);          // v = m 2^e, m in [0.5, 1)
      sd[tid] = ldexp(1.0, -(e >> 1));
    }
  }
  if (bad) atomicOr(&s_bad, 1);
  __syncthreads();
  bad = s_bad != 0;   // (uniform from here on)
  double min_pivot = 0.0;
  if (!bad) {
    // ---- 1. the scaled lower triangle (exact)
    {
      const double dj = sd[ri];
#pragma unroll 8
      for (int i = 0; i < D; ++i)   // (row by row: consecutive work-items, consecutive addresses; the loads of eight rows in flight)
        if (tid <= i) L[i * (i + 1) / 2 + tid] = (S[(size_t)i * D + tid] * sd[i]) * dj;
    }
    __syncthreads();
    // ---- 2a. Cholesky, column by column.  L[j][j] holds the pivot (the square of the factor's diagonal entry) for now.
    min_pivot = __builtin_inf();
    for (int j = 0; j < D; ++j) {
      if (row && tid >= j) {
        const double* Lj = L + j * (j + 1) / 2;
        double a = Li[j];
        int q = 0;
        for (; q + 8 <= j; q += 8) {   // (eight pairs requested together, added in index order)
          double u[8], v[8];
#pragma unroll
          for (int z = 0; z < 8; ++z) u[z] = Li[q + z], v[z] = Lj[q + z];
#pragma unroll
          for (int z = 0; z < 8; ++z) a = __builtin_fma(-u[z], v[z], a);
        }
        for (; q < j; ++q) a = __builtin_fma(-Li[q], Lj[q], a);
        Li[j] = a;
      }
      __syncthreads();
      const double p = L[j * (j + 1) / 2 + j];
      if (!(p > 0.0) || !(p < __builtin_inf())) {   // (the same value for every work-item: the branch is uniform)
        min_pivot = p;
        bad = true;
        break;
      }
      min_pivot = fmin(min_pivot, p);
      if (row && tid > j) Li[j] = Li[j] / sqrt(p);
      __syncthreads();
    }
  }
  if (!bad) {
    // ---- 2b. M = L^-1 in place, from the last column: M[j][j] = 1 / L[j][j], M[i][j] = -(sum_{q = j+1..i} M[i][q] L[q][j]) M[j][j]
    for (int j = D - 1; j >= 0; --j) {
      const double mjj = 1.0 / sqrt(L[j * (j + 1) / 2 + j]);
      double a = 0.0;
      if (row && tid > j) {
        int q = j + 1;
        for (; q + 8 <= tid + 1; q += 8) {
          double u[8], v[8];
#pragma unroll
          for (int z = 0; z < 8; ++z) u[z] = Li[q + z], v[z] = L[(q + z) * (q + z + 1) / 2 + j];
#pragma unroll
          for (int z = 0; z < 8; ++z) a = __builtin_fma(u[z], v[z], a);
        }
        for (; q <= tid; ++q) a = __builtin_fma(Li[q], L[q * (q + 1) / 2 + j], a);
      }
      __syncthreads();
      if (row && tid > j) Li[j] = -a * mjj;
      if (tid == j) Li[j] = mjj;
      __syncthreads();
    }
  }
  for (int c0 = 0; c0 < k && !bad; c0 += COV_KC) {
    const int kc = min(COV_KC, k - c0);
    // y = M^T (M w) for the COV_KC columns w in Wm, into registers (Wm is overwritten with M w on the way)
    auto apply = [&](double (&y)[COV_KC]) {
      double t[COV_KC];
#pragma unroll
      for (int c = 0; c < COV_KC; ++c) t[c] = 0.0;
      if (row)
        for (int q = 0; q <= tid; ++q) {
          const double m = Li[q];
          const double* w = Wm + q * COV_KC;
#pragma unroll
          for (int c = 0; c < COV_KC; ++c) t[c] = __builtin_fma(m, w[c], t[c]);
        }
      __syncthreads();
      if (row) {
#pragma unroll
        for (int c = 0; c < COV_KC; ++c) Wm[tid * COV_KC + c] = t[c];
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < COV_KC; ++c) y[c] = 0.0;
      if (row)
        for (int m = tid; m < D; ++m) {
          const double mm = L[m * (m + 1) / 2 + tid];
          const double* w = Wm + m * COV_KC;
#pragma unroll
          for (int c = 0; c < COV_KC; ++c) y[c] = __builtin_fma(mm, w[c], y[c]);
        }
      __syncthreads();
    };
    double x[COV_KC];
    if (row) {
#pragma unroll
      for (int c = 0; c < COV_KC; ++c) Wm[tid * COV_KC + c] = (c < kc && rows(c0 + c) == tid) ? 1.0 : 0.0;
    }
    __syncthreads();
    apply(x);
    for (int it = 0; it < COV_REFINE; ++it) {
      if (row) {
#pragma unroll
        for (int c = 0; c < COV_KC; ++c) Wm[tid * COV_KC + c] = x[c];
      }
      __syncthreads();
      // residual r = e - S^ x, row `tid`; S^_ij = S_ji d_i d_j is exact, products and sums are error-free transformations
      double hi[COV_KC], lo[COV_KC];
#pragma unroll
      for (int c = 0; c < COV_KC; ++c) {
        hi[c] = (c < kc && rows(c0 + c) == tid) ? 1.0 : 0.0;
        lo[c] = 0.0;
      }
      if (row) {
        const double di = sd[tid];
        double s_next = S[tid];
        for (int j = 0; j < D; ++j) {
          const double s_raw = s_next;
          if (j + 1 < D) s_next = S[(size_t)(j + 1) * D + tid];     // (requested one row ahead)
          const double s = -((s_raw * di) * sd[j]);   // (the symmetric entry: consecutive work-items, consecutive addresses)
          const double* w = Wm + j * COV_KC;
#pragma unroll
          for (int c = 0; c < COV_KC; ++c) cov_dot2_step(s, w[c], hi[c], lo[c]);
        }
      }
      __syncthreads();
      if (row) {
#pragma unroll
        for (int c = 0; c < COV_KC; ++c) Wm[tid * COV_KC + c] = hi[c] + lo[c];
      }
      __syncthreads();
      double dx[COV_KC];
      apply(dx);
#pragma unroll
      for (int c = 0; c < COV_KC; ++c) x[c] += dx[c];
    }
    // ---- 4. the lower triangle of Sigma_K in ascending row order, mirrored
    int a = -1;
    for (int q = 0; q < k; ++q)
      if (row && rows(q) == tid) a = q;
    bool nf = false;
    if (a >= 0) {
      const double da = sd[tid];
#pragma unroll
      for (int c = 0; c < COV_KC; ++c) {
        const int b = c0 + c;
        if (c < kc && a >= b) {
          const double v = (x[c] * da) * sd[rows(b)];
          if (!(fabs(v) < __builtin_inf())) nf = true;
          out[a * k + b] = v;
          out[b * k + a] = v;
        }
      }
    }
    if (nf) atomicOr(&s_bad, 1);
    __syncthreads();
    bad = s_bad != 0;
  }
  if (bad) {
    __syncthreads();
    for (int e = tid; e < k * k; e += COV_THREADS) out[e] = nan;
  }
  if (tid == 0) {
    tail[0] = min_pivot;
    *reinterpret_cast<int*>(tail + 1) = bad ? 1 : 0;
  }
}

__global__ __launch_bounds__(COV_THREADS) void cov_kernel(const CovArgs* __restrict__ args) {
  const CovArgs& A = args[blockIdx.x];
  cov_solve(A.S, A.out, A.out + A.k * A.k, A.D, A.k, CovRowList{A.rows});
}

// Stage one of okvis_ba_landmark_covariance: P = (S0^-1)[0:Dp, 0:Dp], every pose-type column, ceil(Dp / COV_KC) passes over the
// same factor.  One workgroup per window, the LDS of cov_kernel.
struct CovPoseArgs {
  const double* S;   // [D][D] the exported system, full symmetric
  double* P;         // [Dp][Dp]
  double* tail;      // min_pivot | info (int)
  int D, Dp;
};
__global__ __launch_bounds__(COV_THREADS) void cov_pose_kernel(const CovPoseArgs* __restrict__ args) {
  const CovPoseArgs& A = args[blockIdx.x];
  cov_solve(A.S, A.P, A.tail, A.D, A.Dp, CovRowLeading{});
}

// What the assembly launches of okvis_ba_state_covariance write besides linearisation buffers that every okvis_ba_begin rewrites:
// the control record and the IMU terms' preintegration records (a linearisation re-preintegrates a term whose bias has moved).
// Kept before the launches (restore = 0) and put back behind them (restore = 1), so that the solver hands out what it would
// have handed out without the call.  One workgroup per window of the batch; `stride` doubles per window.
constexpr int COV_KEEP_CTRL = 64;
__global__ void cov_keep_kernel(const WinPtrs* __restrict__ wins, double* keep, size_t stride, int max_imu, int restore) {
  const WinPtrs& W = wins[blockIdx.x];
  constexpr int NC = (int)(sizeof(Ctrl) / 8), CD = (int)(sizeof(ImuCacheD) / 8);
  static_assert(NC <= COV_KEEP_CTRL, "the control record's slot");
  double* kc = keep + blockIdx.x * stride;
  double* k0 = kc + COV_KEEP_CTRL;
  double* k1 = k0 + (size_t)max_imu * CD;
  auto c = reinterpret_cast<BA_G double*>(W.ctrl);
  auto i0 = reinterpret_cast<BA_G double*>(W.imu_cache);
  auto i1 = reinterpret_cast<BA_G double*>(W.imu_cache_prev);
  const int n = W.n_imu > 0 ? (W.n_imu < max_imu ? W.n_imu : max_imu) * CD : 0;
  if (restore) {
    for (int i = threadIdx.x; i < NC; i += blockDim.x) c[i] = kc[i];
    for (int i = threadIdx.x; i < n; i += blockDim.x) i0[i] = k0[i], i1[i] = k1[i];
  } else {
    for (int i = threadIdx.x; i < NC; i += blockDim.x) kc[i] = c[i];
    for (int i = threadIdx.x; i < n; i += blockDim.x) k0[i] = i0[i], k1[i] = i1[i];
  }
}

}  // namespace ba
