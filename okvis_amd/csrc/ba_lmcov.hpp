// Landmark covariance (okvis_ba_landmark_covariance, DESIGN.md "Landmark covariance"): the landmark's 3 x 3 diagonal block of the
// inverse of the full undamped normal matrix,
//   G_l = W_l V_l^-1,   Sigma_l = V_l^-1 + G_l^T P[rows_l, rows_l] G_l,
// P the pose-type part of S0^-1 (cov_pose_kernel, ba_cov.hpp), W_l the landmark's 6 x 3 blocks stacked, rows_l their reduced rows,
// V_l^-1 the plain inverse inv3sym forms — the one the elimination used — with one refinement step, so that its error is the
// rounding of its entries rather than cond V x eps.  V and W are read from the linearisation buffer the control record
// names: the one the Schur launch reduced and the solver's own back-substitution reads.
// This file holds lmcov_kernel and, in front of it, the wave core it shares with predcov_kernel (ba_predcov.hpp; DESIGN.md "State
// covariance", "The wave core"): the leading part of the argument record, the wave-level sync, the landmark head, phases 2 and 3
// for NC columns, and the tap kernel of both entries.
// One wave per (window, selected landmark), LMCOV_WAVES of them in a workgroup; nothing is shared between the waves, so there is
// no workgroup barrier and a wave without a landmark leaves at once.  A landmark with n blocks has R = 6 n rows, which may exceed
// the 64 lanes (per-frame extrinsics: 4 frames x 2 cameras = 12 blocks = 72 rows): every phase loops over the rows.
//   1. G [R][3] and the reduced row of every r into LDS (one lane per row);
//   2. T = P[rows, rows] G, one lane per row, the R columns in order; P is bitwise symmetric and is read along its rows
//      (consecutive lanes, consecutive addresses inside a block) — Dp x Dp doubles, resident in L2;
//   3. the six entries of the lower triangle of G^T T: eight lanes per entry take every eighth row in order, their partial sums
//      are added pairwise in a fixed tree; V_l^-1 is added and the triangle mirrored.
// fp64 throughout, explicit fused multiply-adds, no atomics, every sum in an order that depends on the landmark alone: its nine
// numbers have the same bits alone, in any selection and in any range of windows.
// The matrix core is not used: the products have three columns (a 16 x 16 x 4 fp64 tile would carry 13 empty ones), and a wave's
// time is the gather of P and the latency of two dependent phases, not arithmetic (R^2 x 3 = 16 kflop at R = 72).
#pragma once
#include "ba_cov.hpp"
#include "ba_math.hpp"
#include "ba_types.hpp"

namespace ba {

constexpr int LMCOV_THREADS = 256;
constexpr int LMCOV_WAVES = LMCOV_THREADS / 64;
constexpr int LMCOV_MAX_ROWS = MAX_D_LDS;   // a landmark's blocks are distinct pose-type blocks: R <= Dp <= D <= MAX_D_LDS

// ---- The wave core: what lmcov_kernel and predcov_kernel share ----
// The leading part of a window's argument record in either entry (LmcovArgs, PredcovArgs): what the tap kernel needs of it.
struct CovWaveArgs {
  const double* P;     // [Dp][Dp] pose-type part of S0^-1 (NaN throughout when S0 could not be inverted)
  double* tapV;        // null or [n_lm][6]: the referee's copy of V ...
  double* tapW;        // null or [n_pair][18]: ... and of W, from the buffer the kernel reads
  int n;               // items (landmarks, queries) of the window
};

__device__ __forceinline__ void cov_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

// One Newton step X += X (I - V X) on inv3sym's inverse of a symmetric 3 x 3 (both upper-tri 00 01 02 11 12 22), the residual
// accumulated with error-free products and sums (as cov_solve's refinement, ba_cov.hpp).  cond V reaches 5e4 on the referee's
// windows: the cofactors leave cond x eps = 1e-11 in V^-1, the step takes that to the rounding of the entries themselves.
__device__ __forceinline__ void lmcov_refine3(const double* v, double* x) {
  const double V[3][3] = {{v[0], v[1], v[2]}, {v[1], v[3], v[4]}, {v[2], v[4], v[5]}};
  const double X[3][3] = {{x[0], x[1], x[2]}, {x[1], x[3], x[4]}, {x[2], x[4], x[5]}};
  double Rm[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double hi = i == j ? 1.0 : 0.0, lo = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) cov_dot2_step(-V[i][k], X[k][j], hi, lo);
      Rm[i][j] = hi + lo;
    }
  int e = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j, ++e)
      x[e] = X[i][j] + __builtin_fma(X[i][2], Rm[2][j], __builtin_fma(X[i][1], Rm[1][j], X[i][0] * Rm[0][j]));
}

// The landmark head: v = V_l as the linearisation left it, vi = V_l^-1 (inv3sym and the step above; every lane the same numbers) ...
__device__ __forceinline__ void cov_wave_landmark(const BA_G double* Vl, double (&v)[6], double (&vi)[6]) {
#pragma unroll
  for (int e = 0; e < 6; ++e) v[e] = Vl[e];
  inv3sym(v, vi);
  lmcov_refine3(v, vi);
}
// ... and whether the terms show a positive definite V_l: Sylvester's three minors.  (predcov_kernel has these three lines written
// out: with the flag coming back from a function the compiler schedules that kernel differently, same operations, and its stage
// measures 0.9 % slower — profiles/cov_unify_notes.md.)
__device__ __forceinline__ bool cov_wave_positive_definite(const double (&v)[6]) {
  const double m2 = v[0] * v[3] - v[1] * v[1];
  const double det = v[0] * (v[3] * v[5] - v[4] * v[4]) + v[1] * (v[2] * v[4] - v[1] * v[5]) + v[2] * (v[1] * v[4] - v[2] * v[3]);
  return v[0] > 0.0 && m2 > 0.0 && det > 0.0 && det < __builtin_inf();
}

// Phase 2: T [R][NC] = P[rows, rows] X, X [R][NC] and rows [R] in the wave's LDS, one lane per row, the R columns in order.
template <int NC>
__device__ __forceinline__ void cov_wave_gather(const double* P, int Dp, const int* rows, int R, const double* X, double* T, int lane) {
  for (int r = lane; r < R; r += 64) {
    const double* Pr = P + rows[r];
    double t[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) t[j] = 0.0;
    for (int c = 0; c < R; c += 6) {   // (a block's six rows are consecutive: six loads in flight, added in order)
      const size_t base = (size_t)rows[c] * Dp;
      double pc[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) pc[q] = Pr[base + (size_t)q * Dp];
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const double* x = X + NC * (c + q);
#pragma unroll
        for (int j = 0; j < NC; ++j) t[j] = __builtin_fma(pc[q], x[j], t[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) T[NC * r + j] = t[j];
  }
}

// Phase 3: the NC (NC + 1) / 2 entries of the lower triangle of X^T T, entry e = (i, j), i >= j, column by column (00 10 20 11 21
// 22; 00 10 11), on lanes LANES e .. LANES e + LANES - 1 with LANES = 8 (NC = 3) or 16 (NC = 2): each lane takes every LANES-th
// row in order, the partial sums are added pairwise in a fixed tree.  Every lane of entry e returns its sum; `on` is wave-uniform.
template <int NC>
__device__ __forceinline__ double cov_wave_triangle(const double* X, const double* T, int R, int lane, bool on) {
  static_assert(NC == 2 || NC == 3, "two or three columns");
  constexpr int ENTRIES = NC * (NC + 1) / 2, LANES = NC == 3 ? 8 : 16;
  const int e = lane / LANES, seg = lane % LANES;
  int ei, ej;
  if constexpr (NC == 3)
    ei = e < 3 ? e : (e < 5 ? e - 2 : 2), ej = e < 3 ? 0 : (e < 5 ? 1 : 2);
  else
    ei = e == 0 ? 0 : 1, ej = e == 2 ? 1 : 0;
  double part = 0.0;
  if (on && e < ENTRIES)
    for (int r = seg; r < R; r += LANES) part = __builtin_fma(X[NC * r + ei], T[NC * r + ej], part);
#pragma unroll
  for (int m = 1; m < LANES; m <<= 1) part += __shfl_xor(part, m);
  return part;
}

// The referee's taps of V and W: the very buffers the item kernels read.  One workgroup per window; `stride` bytes from one
// window's argument record to the next.
__global__ void cov_tap_kernel(const WinPtrs* __restrict__ wins, const CovWaveArgs* __restrict__ args, size_t stride) {
  const CovWaveArgs& A = *reinterpret_cast<const CovWaveArgs*>(reinterpret_cast<const unsigned char*>(args) + blockIdx.x * stride);
  const WinPtrs& W = wins[blockIdx.x];
  const int acc = W.ctrl->acc & 1;
  if (A.tapV)
    for (int i = threadIdx.x; i < 6 * W.n_lm; i += blockDim.x) A.tapV[i] = W.V[acc][i];
  if (A.tapW)
    for (int i = threadIdx.x; i < 18 * W.n_pair; i += blockDim.x) A.tapW[i] = W.W[acc][i];
}

// ---- The landmark entry ----
struct LmcovArgs : CovWaveArgs {
  const int* sel;      // [n] landmark indices, or null: 0 .. n-1
  double* cov;         // [n][9]
  uint8_t* flags;      // [n]
};

__global__ __launch_bounds__(LMCOV_THREADS) void lmcov_kernel(const WinPtrs* __restrict__ wins, const LmcovArgs* __restrict__ args) {
  __shared__ double s_G[LMCOV_WAVES][LMCOV_MAX_ROWS * 3];
  __shared__ double s_T[LMCOV_WAVES][LMCOV_MAX_ROWS * 3];
  __shared__ int s_row[LMCOV_WAVES][LMCOV_MAX_ROWS];
  const LmcovArgs& A = args[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int item = blockIdx.x * LMCOV_WAVES + wave;
  if (item >= A.n) return;   // (wave-uniform; no workgroup barrier below)
  const WinPtrs& W = wins[blockIdx.y];
  const int acc = W.ctrl->acc & 1;
  const int l = A.sel ? A.sel[item] : item;
  const int p0 = W.lm_pair_begin[l], p1 = W.lm_pair_begin[l + 1];
  const int R = 6 * (p1 - p0), Dp = W.Dp;
  double* const G = s_G[wave];
  double* const T = s_T[wave];
  int* const rows = s_row[wave];
  const double nan = __builtin_nan(""), inf = __builtin_inf();

  double v[6], vi[6];
  cov_wave_landmark(W.V[acc] + 6 * (size_t)l, v, vi);
  const bool pd = cov_wave_positive_definite(v);
  bool ok = R > 0 && R <= LMCOV_MAX_ROWS && pd;

  if (ok) {
    // ---- 1. G = W V^-1 and the reduced rows
    bool outside = false;
    for (int r = lane; r < R; r += 64) {
      const int pr = r / 6, rr = r - 6 * pr, p = p0 + pr;
      const int off = W.pair_off[p];
      if (off < 0 || off + 6 > Dp) outside = true;
      const BA_G double* w = W.W[acc] + (size_t)p * 18 + rr * 3;
      const double w0 = w[0], w1 = w[1], w2 = w[2];
      rows[r] = off + rr;
      G[3 * r + 0] = __builtin_fma(w2, vi[2], __builtin_fma(w1, vi[1], w0 * vi[0]));
      G[3 * r + 1] = __builtin_fma(w2, vi[4], __builtin_fma(w1, vi[3], w0 * vi[1]));
      G[3 * r + 2] = __builtin_fma(w2, vi[5], __builtin_fma(w1, vi[4], w0 * vi[2]));
    }
    if (__any(outside)) ok = false;   // (never, by the index build: a pair's block is a free pose-type block)
  }
  if (ok) {
    cov_wave_sync();
    cov_wave_gather<3>(A.P, Dp, rows, R, G, T, lane);   // ---- 2. T = P[rows, rows] G
    cov_wave_sync();
  }
  // ---- 3. the lower triangle of G^T T, entry e on lanes 8 e .. 8 e + 7 in inv3sym's order read as 00 10 20 11 21 22; V_l^-1 is added
  const int e = lane >> 3;
  const double part = cov_wave_triangle<3>(G, T, R, lane, ok);
  const double vie = e == 0 ? vi[0] : (e == 1 ? vi[1] : (e == 2 ? vi[2] : (e == 3 ? vi[3] : (e == 4 ? vi[4] : vi[5]))));
  const double val = vie + part;
  if (__any(e < 6 && !(fabs(val) < inf))) ok = false;
  // entry k = 3 a + b of the result is entry (max, min) of the triangle
  const int k = lane < 9 ? lane : 0, ka = k / 3, kb = k - 3 * ka;
  const int hi = ka > kb ? ka : kb, lo = ka > kb ? kb : ka;
  const double o = __shfl(val, 8 * (lo == 0 ? hi : (lo == 1 ? hi + 2 : 5)));
  if (lane < 9) A.cov[(size_t)item * 9 + lane] = ok ? o : nan;
  if (lane == 0) A.flags[item] = ok ? 0 : 1;
}

}  // namespace ba
