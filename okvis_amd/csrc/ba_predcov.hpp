// Predicted measurement covariance (okvis_ba_predicted_measurement, DESIGN.md "Predicted measurement covariance"): the 2 x 2
// covariance of a landmark's predicted pixel under the joint uncertainty of the landmark, the pose and the extrinsics it is seen
// through.  A query (lm, pose, ext, cam) has the meaning of an observation row; it need not be one of the window's.  With V_l, W_l,
// G_l = W_l V_l^-1, rows_l and P exactly as lmcov_kernel (ba_lmcov.hpp) takes them, uv the projection and J_l (2 x 3), J_p, J_e
// (2 x 6) its derivatives in the solver's tangent coordinates (predcov_project below: reproj_linearize, ba_math.hpp, with unit
// information and the sign of the residual removed), rows_x the reduced rows of the query's free pose / extrinsics blocks and R = rows_l u rows_x:
//   A = J_x E_x - J_l G_l^T E_l   (2 x |R|),      U = J_l V_l^-1 J_l^T + A P[R, R] A^T   (2 x 2)
// = J Sigma J^T for J = [J_l J_p J_e] and Sigma the block of the inverse of the full undamped normal matrix: both terms positive
// semi-definite, the large world-frame terms cancel inside A (a landmark is tight against the cameras that see it, the window as
// a whole is loose against the world) before P is applied.  The reference computes nothing of the kind.
// One wave per (window, query), PREDCOV_WAVES of them in a workgroup; the waves share nothing: no workgroup barrier, no atomics, and
// a wave without a query leaves at once.  Every lane forms V_l^-1, the projection and the three Jacobians (the same numbers in
// every lane); lane 0 puts uv and the Jacobians into the wave's LDS slab, where the phases below index them by row.
//   1. A [|R|][2] and the reduced row of every r into LDS, one lane per row: the landmark's rows first, J_l G^T = (W N)^T with
//      N = V_l^-1 J_l^T solved once per wave (predcov_solve3: G itself is never formed; a query block that is also one of the
//      landmark's adds its J_x there), then the query blocks the landmark does not touch;
//   2. T = P[R, R] A^T, one lane per row, the |R| columns in order; P is bitwise symmetric and is read along its rows;
//   3. the three entries of the lower triangle of A T: sixteen lanes per entry take every sixteenth row in order, their partial
//      sums are added pairwise in a fixed tree; J_l V_l^-1 J_l^T = J_l N is added and the triangle mirrored.
// |R| reaches 84 with per-frame extrinsics (12 landmark blocks + 2 query blocks): every phase loops over the rows.
// fp64 throughout, explicit fused multiply-adds, every sum in an order that depends on the query alone: its numbers have the same
// bits alone, in any list and in any range of windows.  The matrix core is not used: the products have two columns.
// This file holds what is the query's own: the projection (predcov_project), N (predcov_solve3), phase 1 and the flags.  The
// landmark head, phases 2 and 3, the wave-level sync and the tap kernel are the wave core in ba_lmcov.hpp, with NC = 2.
#pragma once
#include "ba_lmcov.hpp"
#include "ba_math.hpp"
#include "ba_types.hpp"

namespace ba {

constexpr int PREDCOV_THREADS = 256;
constexpr int PREDCOV_WAVES = PREDCOV_THREADS / 64;
constexpr int PREDCOV_MAX_ROWS = MAX_D_LDS;   // R is a set of rows of distinct pose-type blocks: |R| <= Dp <= D <= MAX_D_LDS
constexpr int PREDCOV_JAC = 30;               // J_l [2][3] | J_p [2][6] | J_e [2][6], row-major
constexpr uint8_t PREDCOV_NO_COV = 1, PREDCOV_NO_PROJECTION = 2;

struct PredcovArgs : CovWaveArgs {
  const int4* q;       // [n] lm, pose, ext, cam
  double* uv;          // [n][2]
  double* cov;         // [n][4]
  uint8_t* flags;      // [n]
  double* jac;         // null or [n][PREDCOV_JAC]: the Jacobians the wave formed
};

// The predicted pixel and its minimal Jacobians: the algebra of reproj_linearize (ba_math.hpp; ReprojectionError.hpp:87-242) for the
// projection itself — unit information, no measurement, the sign of the residual removed — with its rule for a point that does
// not project: the projection undefined (|z| < 1e-12, PinholeCamera.hpp:155-157, or the distortion refuses) or the point less
// than 0.2 in front of the camera (ReprojectionError.hpp:143-151).  Every output is written on every path.
struct PredProj {
  double uv[2];
  double Jl[6];    // 2 x 3, the landmark's first three coordinates
  double Jp[12];   // 2 x 6, T_WS
  double Je[12];   // 2 x 6, T_SC
};
__device__ __forceinline__ bool predcov_project(const double* pose, const double* ext, const double* lm, const double* intr, int model, PredProj& o) {
  double C_WS[9], C_SC[9];
  qrot(pose + 3, C_WS);
  qrot(ext + 3, C_SC);
  const double w = lm[3];
  const double dW[3] = {lm[0] - pose[0] * w, lm[1] - pose[1] * w, lm[2] - pose[2] * w};
  double pS[3];
  mat3_Tvec(C_WS, dW, pS);
  const double eS[3] = {pS[0] - ext[0] * w, pS[1] - ext[1] * w, pS[2] - ext[2] * w};
  double pC[3];
  mat3_Tvec(C_SC, eS, pC);
  // projectHomogeneous (PinholeCamera.hpp:357-378): w < 0 -> project(-head), Jacobian sign kept
  const double sgn = w < 0 ? -1.0 : 1.0;
  const double x = sgn * pC[0], y = sgn * pC[1], z = sgn * pC[2];
  bool good = fabs(z) >= 1.0e-12;
  const double rz = good ? 1.0 / z : 0.0, rz2 = rz * rz;
  double dd[2] = {0, 0}, Jd[4] = {1, 0, 0, 1};
  if (!distort(model, intr + 4, x * rz, y * rz, dd, Jd)) good = false;
  if (fabs(w) > 1.0e-8 && pC[2] / w < 0.2) good = false;
  const double fu = intr[0], fv = intr[1];
  o.uv[0] = fu * dd[0] + intr[2];
  o.uv[1] = fv * dd[1] + intr[3];
  // Jc = J_project (2 x 3) (PinholeCamera.hpp:196-206)
  const double Jc[6] = {fu * Jd[0] * rz, fu * Jd[1] * rz, -fu * (x * Jd[0] + y * Jd[1]) * rz2,
                        fv * Jd[2] * rz, fv * Jd[3] * rz, -fv * (x * Jd[2] + y * Jd[3]) * rz2};
  // B = Jc C_SC^T;  J_l = B C_WS^T;  J_p = -J_l [I w, -[dW]x];  J_e = -B [I w, -[eS]x]
  double B[6];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      B[3 * i + j] = Jc[3 * i] * C_SC[3 * j] + Jc[3 * i + 1] * C_SC[3 * j + 1] + Jc[3 * i + 2] * C_SC[3 * j + 2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o.Jl[3 * i + j] = B[3 * i] * C_WS[3 * j] + B[3 * i + 1] * C_WS[3 * j + 1] + B[3 * i + 2] * C_WS[3 * j + 2];
    const double a0 = o.Jl[3 * i], a1 = o.Jl[3 * i + 1], a2 = o.Jl[3 * i + 2];
    o.Jp[6 * i + 0] = -w * a0;
    o.Jp[6 * i + 1] = -w * a1;
    o.Jp[6 * i + 2] = -w * a2;
    o.Jp[6 * i + 3] = a1 * dW[2] - a2 * dW[1];
    o.Jp[6 * i + 4] = a2 * dW[0] - a0 * dW[2];
    o.Jp[6 * i + 5] = a0 * dW[1] - a1 * dW[0];
    const double b0 = B[3 * i], b1 = B[3 * i + 1], b2 = B[3 * i + 2];
    o.Je[6 * i + 0] = -w * b0;
    o.Je[6 * i + 1] = -w * b1;
    o.Je[6 * i + 2] = -w * b2;
    o.Je[6 * i + 3] = b1 * eS[2] - b2 * eS[1];
    o.Je[6 * i + 4] = b2 * eS[0] - b0 * eS[2];
    o.Je[6 * i + 5] = b0 * eS[1] - b1 * eS[0];
  }
  return good;
}

// N = V^-1 J_l^T (3 x 2, N[3 j + k] = column j): X J_l^T with X the refined inverse, then one step N += X (J_l^T - V N), the
// residual accumulated with error-free products and sums (as lmcov_refine3).  J_l annihilates the ray through the landmark, the
// direction in which V^-1 is largest: the plain product keeps cond V x eps of the entries of X (measured on the referee's
// windows: 1e-12 of U), the step takes N to the rounding of its own entries.
__device__ __forceinline__ void predcov_solve3(const double* v, const double* x, const double* Jl, double* N) {
  const double V[3][3] = {{v[0], v[1], v[2]}, {v[1], v[3], v[4]}, {v[2], v[4], v[5]}};
  const double X[3][3] = {{x[0], x[1], x[2]}, {x[1], x[3], x[4]}, {x[2], x[4], x[5]}};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    double n0[3], res[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) n0[i] = __builtin_fma(X[i][2], Jl[3 * j + 2], __builtin_fma(X[i][1], Jl[3 * j + 1], X[i][0] * Jl[3 * j]));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double hi = Jl[3 * j + i], lo = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) cov_dot2_step(-V[i][k], n0[k], hi, lo);
      res[i] = hi + lo;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) N[3 * j + i] = n0[i] + __builtin_fma(X[i][2], res[2], __builtin_fma(X[i][1], res[1], X[i][0] * res[0]));
  }
}

__global__ __launch_bounds__(PREDCOV_THREADS) void predcov_kernel(const WinPtrs* __restrict__ wins, const PredcovArgs* __restrict__ args) {
  __shared__ double s_A[PREDCOV_WAVES][PREDCOV_MAX_ROWS * 2];
  __shared__ double s_T[PREDCOV_WAVES][PREDCOV_MAX_ROWS * 2];
  __shared__ double s_J[PREDCOV_WAVES][PREDCOV_JAC + 2];
  __shared__ int s_row[PREDCOV_WAVES][PREDCOV_MAX_ROWS];
  const PredcovArgs& Q = args[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int item = blockIdx.x * PREDCOV_WAVES + wave;
  if (item >= Q.n) return;   // (wave-uniform; no workgroup barrier below)
  const WinPtrs& W = wins[blockIdx.y];
  const int acc = W.ctrl->acc & 1;
  const int4 q = Q.q[item];
  const int l = q.x;
  const int p0 = W.lm_pair_begin[l], p1 = W.lm_pair_begin[l + 1];
  const int Rl = 6 * (p1 - p0), Dp = W.Dp;
  const int off_p = W.pose_off[q.y], off_e = W.pose_off[q.z];   // reduced offset, or -1: a fixed block has no rows
  double* const A = s_A[wave];
  double* const T = s_T[wave];
  double* const J = s_J[wave];
  int* const rows = s_row[wave];
  const double nan = __builtin_nan(""), inf = __builtin_inf();

  double v[6], vi[6];
  cov_wave_landmark(W.V[acc] + 6 * (size_t)l, v, vi);
  // (cov_wave_positive_definite(v), written out: ba_lmcov.hpp says why)
  const double m2 = v[0] * v[3] - v[1] * v[1];
  const double det = v[0] * (v[3] * v[5] - v[4] * v[4]) + v[1] * (v[2] * v[4] - v[1] * v[5]) + v[2] * (v[1] * v[4] - v[2] * v[3]);
  bool ok = Rl > 0 && Rl <= PREDCOV_MAX_ROWS && v[0] > 0.0 && m2 > 0.0 && det > 0.0 && det < inf;

  // the projection and its Jacobians at the state the linearisation buffer `acc` belongs to
  PredProj lin;
  bool projects;
  {
    const BA_G double* pose = W.pose[acc] + 7 * (size_t)q.y;
    const BA_G double* ext = W.pose[acc] + 7 * (size_t)q.z;
    const BA_G double* lm = W.lm[acc] + 4 * (size_t)l;
    double Pq[7], Eq[7], intr[12];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      Pq[i] = pose[i];
      Eq[i] = ext[i];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) intr[i] = W.cam_intr[12 * q.w + i];
    const double L4[4] = {lm[0], lm[1], lm[2], lm[3]};
    projects = predcov_project(Pq, Eq, L4, intr, W.cam_model[q.w], lin);
  }
  double Jl[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) Jl[i] = lin.Jl[i];
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) J[i] = Jl[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      J[6 + i] = lin.Jp[i];
      J[18 + i] = lin.Je[i];
    }
    J[PREDCOV_JAC] = lin.uv[0], J[PREDCOV_JAC + 1] = lin.uv[1];
  }
  cov_wave_sync();
  if (lane < 2) Q.uv[(size_t)item * 2 + lane] = projects ? J[PREDCOV_JAC + lane] : nan;
  if (Q.jac && lane < PREDCOV_JAC) Q.jac[(size_t)item * PREDCOV_JAC + lane] = projects ? J[lane] : nan;
  double N[6];   // V_l^-1 J_l^T: J_l G^T = (W N)^T and J_l V_l^-1 J_l^T = J_l N
  predcov_solve3(v, vi, Jl, N);
  bool no_cov = !ok;   // the landmark's side: no pair, or V_l not positive definite
  if (!projects) ok = false;

  int R = 0;
  if (ok) {
    // ---- 1. A = J_x E_x - J_l G^T E_l and the reduced rows: the landmark's rows ...
    bool outside = false, has_p = false, has_e = false;
    for (int r = lane; r < Rl; r += 64) {
      const int pr = r / 6, rr = r - 6 * pr, p = p0 + pr;
      const int off = W.pair_off[p];
      if (off < 0 || off + 6 > Dp) outside = true;
      const BA_G double* w = W.W[acc] + (size_t)p * 18 + rr * 3;
      const double w0 = w[0], w1 = w[1], w2 = w[2];
      double a0 = -__builtin_fma(w2, N[2], __builtin_fma(w1, N[1], w0 * N[0]));
      double a1 = -__builtin_fma(w2, N[5], __builtin_fma(w1, N[4], w0 * N[3]));
      if (off == off_p) {
        has_p = true;
        a0 += J[6 + rr], a1 += J[12 + rr];
      }
      if (off == off_e) {
        has_e = true;
        a0 += J[18 + rr], a1 += J[24 + rr];
      }
      rows[r] = off + rr;
      A[2 * r + 0] = a0, A[2 * r + 1] = a1;
    }
    // ... then the query's free blocks the landmark has no pair with (pose before extrinsics)
    R = Rl;
    const bool add_p = off_p >= 0 && !__any(has_p), add_e = off_e >= 0 && !__any(has_e);
    if (off_p + 6 > Dp || off_e + 6 > Dp) outside = true;   // (never, by the index build: a free pose-type block lies below Dp)
    if (R + (add_p ? 6 : 0) + (add_e ? 6 : 0) > PREDCOV_MAX_ROWS) outside = true;   // (never: distinct blocks, |R| <= Dp)
    if (!__any(outside)) {
      if (add_p) {
        if (lane < 6) {
          rows[R + lane] = off_p + lane;
          A[2 * (R + lane) + 0] = J[6 + lane], A[2 * (R + lane) + 1] = J[12 + lane];
        }
        R += 6;
      }
      if (add_e) {
        if (lane < 6) {
          rows[R + lane] = off_e + lane;
          A[2 * (R + lane) + 0] = J[18 + lane], A[2 * (R + lane) + 1] = J[24 + lane];
        }
        R += 6;
      }
    } else {
      ok = false, no_cov = true;
    }
  }
  if (ok) {
    cov_wave_sync();
    cov_wave_gather<2>(Q.P, Dp, rows, R, A, T, lane);   // ---- 2. T = P[R, R] A^T
    cov_wave_sync();
  }
  // ---- 3. the lower triangle of A T, entry e on lanes 16 e .. 16 e + 15 in the order 00 10 11
  const int e = lane >> 4;
  const double part = cov_wave_triangle<2>(A, T, R, lane, ok);
  // J_l V_l^-1 J_l^T = J_l N
  const double l00 = __builtin_fma(Jl[2], N[2], __builtin_fma(Jl[1], N[1], Jl[0] * N[0]));
  const double l10 = __builtin_fma(Jl[5], N[2], __builtin_fma(Jl[4], N[1], Jl[3] * N[0]));
  const double l11 = __builtin_fma(Jl[5], N[5], __builtin_fma(Jl[4], N[4], Jl[3] * N[3]));
  const double val = (e == 0 ? l00 : (e == 1 ? l10 : l11)) + part;
  if (ok && __any(e < 3 && !(fabs(val) < inf))) ok = false, no_cov = true;
  // entry k = 2 a + b of the result is entry (max, min) of the triangle: 00 | 10 | 10 | 11
  const double o = __shfl(val, 16 * (lane == 0 ? 0 : (lane == 3 ? 2 : 1)));
  if (lane < 4) Q.cov[(size_t)item * 4 + lane] = ok ? o : nan;
  if (lane == 0) Q.flags[item] = (uint8_t)((no_cov ? PREDCOV_NO_COV : 0) | (projects ? 0 : PREDCOV_NO_PROJECTION));
}

}  // namespace ba
