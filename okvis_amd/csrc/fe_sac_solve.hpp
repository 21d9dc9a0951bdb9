// The two minimal solvers of Frontend::runRansac2d2d (okvis_frontend/src/Frontend.cpp:645-810) on the device
// (include/okvis_amd_frontend.h: okvis_fe_sac_solve): a rotation from two correspondences (FrameRotationOnlySacProblem) and a
// relative pose from five correspondences plus three that pick the pose (FrameRelativePoseSacProblem, STEWENIUS).  The solvers
// are OpenGV's and OpenGV's source is not part of the reference tree: both are stated from their published mathematical
// definitions and are NOT pinned to OpenGV ("2D-2D hypotheses").
//
// Convention (the consensus entry's): a point of frame 2 is R12 p2 + t12 in frame 1, R f2 ~ f1, f1^T E f2 = 0, E = [t12]x R12.
//
// Two-point rotation (sac2_rotation): the orthonormal frames (a1, a2, a3) = (f1_i, (f1_i x f1_j)/|.|, a1 x a2) and (b1, b2, b3)
// alike from frame 2; R = a1 b1^T + a2 b2^T + a3 b3^T, every product and sum rounded on its own (BA_NO_CONTRACT).
//
// Five-point relative pose (sac5_wave), Nister's route with a polish on the definition:
//   1  null space of the 5x9 epipolar matrix: Householder reflections on [A^T | I9], lanes take the 14 columns
//   2  the ten cubics (det E = 0, E E^T E - 1/2 tr(E E^T) E = 0) in E = x B0 + y B1 + z B2 + B3: lanes take the constraints,
//      each expands its 20 coefficients (sac5_cubic)
//   3  Gauss-Jordan on the 10x20 coefficient matrix in LDS, partial pivoting, lanes take columns
//   4  the 3x3 matrix of polynomials in z and its determinant of degree ten (sac5_poly10)
//   5  real roots: p on [-1, 1] and the reversed polynomial on [-1, 1] for |z| > 1 (two teams of lanes).  The roots of a
//      polynomial lie one each between consecutive roots of its derivative where the sign changes, so ten levels (degree 1..10)
//      of SAC5_BISECT bisection steps and SAC5_NEWTON guarded Newton steps, lanes take the intervals: every loop has a
//      compile-time count
//   6  per root: (x, y) from the 3x3 matrix at the root, then SAC5_POLISH Gauss-Newton steps on the ten cubics themselves in
//      the unit coefficient vector of the null space basis (sac5_polish), so that what is left is the rounding of the
//      definition and not of steps 3 to 5
//   7  per (root, decomposition): t = the left null vector, R = 2 cof(E) -+ sqrt(2) [t]x E for |E|_F = 1 (the two rotations
//      of U W V^T / U W^T V^T), one polar step on R, the ray parameters and scores of all eight correspondences (sac5_candidate)
//   8  the passing candidate with the smallest score sum
// No workgroup barrier, no atomics, all fp64.  One wave per sample, its working set in the wave's own LDS slab (SOLVE_SLAB
// doubles); rotation-only samples go 64 to a wave, one per lane.
//
// sac5_wave is ONE source for the device and the host: the device calls it with (lane, 64) and the loops "for l = lane; l < N;
// l += stride" spread over the wave, a plain host compiler calls it with (0, 1) and runs them in order.  SOLVE_SYNC orders the
// wave's LDS traffic on the device and is nothing on the host.  Code outside such loops is wave-uniform.
#pragma once
#include "fe_sac.hpp"

namespace fe {

constexpr int SAC5_BISECT = 30;  // bisection steps per level: 2^-29 of the interval, then
constexpr int SAC5_NEWTON = 2;   // guarded Newton steps
constexpr int SAC5_POLISH = 3;   // Gauss-Newton steps on the definition
constexpr int SOLVE_MAX_ROOTS = OKVIS_FE_SAC_MAX_ROOTS;

// the wave's slab, offsets in doubles
constexpr int SV_CORR = 0;      // [8][8] the sample's correspondences: f1 (3), f2 (3), sigma1, sigma2
constexpr int SV_MAT = 64;      // [14][9] columns of [A^T | I9], then [10][20] the coefficient matrix
constexpr int SV_B = 264;       // [4][9] null space basis, orthonormal
constexpr int SV_ROWS = 300;    // [3][13] the rows of the 3x3 polynomial matrix: x part (4), y part (4), constant part (5), ascending
constexpr int SV_P = 340;       // [11] the polynomial of degree ten, ascending
constexpr int SV_POLY = 352;    // [2][66] per team the derivative chain: degree d at SV_OFF(d)
constexpr int SV_PTS = 484;     // [2][2][12] per team two buffers of interval ends
constexpr int SV_FLAG = 532;    // [2][12] per team: interval i of the last level holds a root
constexpr int SV_SLOT = 556;    // [10] team * 16 + interval of root r; [10] the number of roots
constexpr int SV_C = 568;       // [10][4] unit coefficient vectors of the roots
constexpr int SV_E = 608;       // [10][9] the essential matrices, unit Frobenius norm
constexpr int SV_CAND = 698;    // [40][12] the candidates' transformations
constexpr int SV_SUM = 1178;    // [40] their score sums, +inf for a candidate that does not pass
constexpr int SOLVE_SLAB = 1218;

#if defined(__HIP_DEVICE_COMPILE__)
#define SOLVE_SYNC()                                          \
  do {                                                        \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
    __builtin_amdgcn_wave_barrier();                          \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
  } while (0)
#else
#define SOLVE_SYNC() \
  do {               \
  } while (0)
#endif

BA_HD double sac_nan() { return __builtin_nan(""); }
BA_HD bool sac_finite(double x) { return x - x == 0.0; }

BA_HD void sac_cross(const double* u, const double* v, double* w) {
  BA_NO_CONTRACT
  w[0] = u[1] * v[2] - u[2] * v[1];
  w[1] = u[2] * v[0] - u[0] * v[2];
  w[2] = u[0] * v[1] - u[1] * v[0];
}

// ---- two points ---------------------------------------------------------------------------------------------------------------------
// (a1, a2, a3) of one frame; false when the cross product's norm is zero or not finite
BA_HD bool sac2_frame(const double* fi, const double* fj, double* a2, double* a3) {
  BA_NO_CONTRACT
  double c[3];
  sac_cross(fi, fj, c);
  const double n = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  if (!(n > 0.0) || !sac_finite(n)) return false;
  a2[0] = c[0] / n, a2[1] = c[1] / n, a2[2] = c[2] / n;
  sac_cross(fi, a2, a3);
  return true;
}

// R [9] row-major from the sample (i, j); false (R untouched) for an invalid sample.  The caller checks i != j.
BA_HD bool sac2_rotation(const double* f1i, const double* f1j, const double* f2i, const double* f2j, double* R) {
  BA_NO_CONTRACT
  double a2[3], a3[3], b2[3], b3[3];
  if (!sac2_frame(f1i, f1j, a2, a3) || !sac2_frame(f2i, f2j, b2, b3)) return false;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (f1i[r] * f2i[c] + a2[r] * b2[c]) + a3[r] * b3[c];
  return true;
}

// ---- five points: the ten cubics ----------------------------------------------------------------------------------------------------
// Monomials of degree three in (x, y, z, 1) = variables (0, 1, 2, 3), in the column order of the elimination: the first ten are
// what Gauss-Jordan removes, the last ten are (x, y, 1) times powers of z.
//   0 x^3  1 y^3  2 x^2y  3 xy^2  4 x^2z  5 x^2  6 y^2z  7 y^2  8 xyz  9 xy | 10 xz^2  11 xz  12 x  13 yz^2  14 yz  15 y  16 z^3  17 z^2  18 z  19 1
constexpr int SAC5_MONO[20][3] = {{0, 0, 0}, {1, 1, 1}, {0, 0, 1}, {0, 1, 1}, {0, 0, 2}, {0, 0, 3}, {1, 1, 2}, {1, 1, 3}, {0, 1, 2}, {0, 1, 3},
                                  {0, 2, 2}, {0, 2, 3}, {0, 3, 3}, {1, 2, 2}, {1, 2, 3}, {1, 3, 3}, {2, 2, 2}, {2, 2, 3}, {2, 3, 3}, {3, 3, 3}};
constexpr int sac5_i2(int i, int j) { return i <= j ? 4 * i - i * (i - 1) / 2 + (j - i) : 4 * j - j * (j - 1) / 2 + (i - j); }
constexpr int sac5_i3(int i, int j, int k) {
  int a = i, b = j, c = k, t = 0;
  if (a > b) t = a, a = b, b = t;
  if (b > c) t = b, b = c, c = t;
  if (a > b) t = a, a = b, b = t;
  for (int m = 0; m < 20; ++m)
    if (SAC5_MONO[m][0] == a && SAC5_MONO[m][1] == b && SAC5_MONO[m][2] == c) return m;
  return -1;
}
template <int I, int J>
struct Sac5I2 { static constexpr int v = sac5_i2(I, J); };
template <int I, int J, int K>
struct Sac5I3 { static constexpr int v = sac5_i3(I, J, K); };

// out (degree 2, 10 coefficients) += sgn * a * b, a and b linear (4 coefficients); indices are compile-time throughout
template <int I, int J>
BA_HD void sac5_mul11_term(const double* a, const double* b, double sgn, double* out) {
  BA_NO_CONTRACT
  out[Sac5I2<I, J>::v] = out[Sac5I2<I, J>::v] + sgn * (a[I] * b[J]);
  if constexpr (J < 3) sac5_mul11_term<I, J + 1>(a, b, sgn, out);
  else if constexpr (I < 3) sac5_mul11_term<I + 1, 0>(a, b, sgn, out);
}
BA_HD void sac5_mul11(const double* a, const double* b, double sgn, double* out) { sac5_mul11_term<0, 0>(a, b, sgn, out); }

// out (degree 3, 20 coefficients) += p * l, p of degree 2 over the pairs I <= J, l linear
template <int I, int J, int K>
BA_HD void sac5_mul21_term(const double* p, const double* l, double* out) {
  BA_NO_CONTRACT
  out[Sac5I3<I, J, K>::v] = out[Sac5I3<I, J, K>::v] + p[Sac5I2<I, J>::v] * l[K];
  if constexpr (K < 3) sac5_mul21_term<I, J, K + 1>(p, l, out);
  else if constexpr (J < 3) sac5_mul21_term<I, J + 1, 0>(p, l, out);
  else if constexpr (I < 3) sac5_mul21_term<I + 1, I + 1, 0>(p, l, out);
}
BA_HD void sac5_mul21(const double* p, const double* l, double* out) { sac5_mul21_term<0, 0, 0>(p, l, out); }

// the linear polynomial of entry (r, c) of E = sum_i c_i B_i
BA_HD void sac5_entry(const double* B, int r, int c, double* l) {
  for (int i = 0; i < 4; ++i) l[i] = B[9 * i + 3 * r + c];
}

// Constraint q of the ten: q = 3 r + c < 9 is entry (r, c) of E E^T E - 1/2 tr(E E^T) E, q = 9 is det E; its 20 coefficients
// in the order of SAC5_MONO go to row[0..19].
BA_HD void sac5_cubic(const double* B, int q, double* row) {
  BA_NO_CONTRACT
  double acc[20];
  for (int m = 0; m < 20; ++m) acc[m] = 0.0;
  double u[4], v[4], w[4];
  if (q < 9) {
    const int r = q / 3, c = q - 3 * r;
    double half_tr[10];
    for (int m = 0; m < 10; ++m) half_tr[m] = 0.0;
    for (int a = 0; a < 3; ++a)
      for (int m = 0; m < 3; ++m) {
        sac5_entry(B, a, m, u);
        sac5_mul11(u, u, 0.5, half_tr);
      }
    for (int k = 0; k < 3; ++k) {
      double lam[10];  // (E E^T - 1/2 tr I)(r, k)
      for (int m = 0; m < 10; ++m) lam[m] = 0.0;
      for (int m = 0; m < 3; ++m) {
        sac5_entry(B, r, m, u);
        sac5_entry(B, k, m, v);
        sac5_mul11(u, v, 1.0, lam);
      }
      if (k == r)
        for (int m = 0; m < 10; ++m) lam[m] = lam[m] - half_tr[m];
      sac5_entry(B, k, c, w);
      sac5_mul21(lam, w, acc);
    }
  } else {
    for (int a = 0; a < 3; ++a) {  // E(0, a) * cofactor: columns (a + 1) % 3, (a + 2) % 3 of rows 1, 2 in cyclic order
      const int b = (a + 1) % 3, c = (a + 2) % 3;
      double minor[10];
      for (int m = 0; m < 10; ++m) minor[m] = 0.0;
      sac5_entry(B, 1, b, u);
      sac5_entry(B, 2, c, v);
      sac5_mul11(u, v, 1.0, minor);
      sac5_entry(B, 1, c, u);
      sac5_entry(B, 2, b, v);
      sac5_mul11(u, v, -1.0, minor);
      sac5_entry(B, 0, a, w);
      sac5_mul21(minor, w, acc);
    }
  }
  for (int m = 0; m < 20; ++m) row[m] = acc[m];
}

// ---- five points: the polynomial of degree ten --------------------------------------------------------------------------------------
// out[0 .. NA + NB - 2] (+)= sgn * a * b for polynomials with NA and NB ascending coefficients
template <int NA, int NB>
BA_HD void sac5_polymul(const double* a, const double* b, double sgn, double* out) {
  BA_NO_CONTRACT
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) out[i + j] = out[i + j] + sgn * (a[i] * b[j]);
}

// rows: [3][13] (x part 4, y part 4, constant part 5); p[11] = det, ascending
BA_HD void sac5_poly10(const double* rows, double* p) {
  BA_NO_CONTRACT
  double k[13], l[13], m[13];
#pragma unroll
  for (int i = 0; i < 13; ++i) k[i] = rows[i], l[i] = rows[13 + i], m[i] = rows[26 + i];
  double c0[8], c1[8], c2[7];
#pragma unroll
  for (int i = 0; i < 8; ++i) c0[i] = 0.0, c1[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 7; ++i) c2[i] = 0.0;
  sac5_polymul<4, 5>(l + 4, m + 8, 1.0, c0);   // l_y m_1 - l_1 m_y
  sac5_polymul<5, 4>(l + 8, m + 4, -1.0, c0);
  sac5_polymul<5, 4>(l + 8, m, 1.0, c1);       // l_1 m_x - l_x m_1
  sac5_polymul<4, 5>(l, m + 8, -1.0, c1);
  sac5_polymul<4, 4>(l, m + 4, 1.0, c2);       // l_x m_y - l_y m_x
  sac5_polymul<4, 4>(l + 4, m, -1.0, c2);
#pragma unroll
  for (int i = 0; i < 11; ++i) p[i] = 0.0;
  sac5_polymul<4, 8>(k, c0, 1.0, p);
  sac5_polymul<4, 8>(k + 4, c1, 1.0, p);
  sac5_polymul<5, 7>(k + 8, c2, 1.0, p);
}

constexpr int SV_OFF(int d) { return d * (d + 1) / 2 - 1; }  // degree d of the derivative chain: d + 1 coefficients

template <int D>
BA_HD double sac5_horner(const double* q, double x) {
  BA_NO_CONTRACT
  double s = q[D];
#pragma unroll
  for (int j = D - 1; j >= 0; --j) s = s * x + q[j];
  return s;
}

// The root of the polynomial qs of degree D (ascending) on [a, b] when its sign changes there: SAC5_BISECT bisection steps, then
// SAC5_NEWTON guarded Newton steps.  *found = the sign changes; without one the result is not meant to be used.
template <int D>
BA_HD double sac_interval_root(const double* qs, double a, double b, bool* found) {
  BA_NO_CONTRACT
  double q[D + 1], dq[D];
#pragma unroll
  for (int j = 0; j <= D; ++j) q[j] = qs[j];
#pragma unroll
  for (int j = 0; j < D; ++j) dq[j] = (double)(j + 1) * q[j + 1];
  const bool fa = sac5_horner<D>(q, a) > 0.0, fb = sac5_horner<D>(q, b) > 0.0;
  double lo = a, hi = b;
  for (int it = 0; it < SAC5_BISECT; ++it) {
    const double mid = 0.5 * (lo + hi);
    const bool fm = sac5_horner<D>(q, mid) > 0.0;
    if (fm == fa) lo = mid;
    else hi = mid;
  }
  double x = 0.5 * (lo + hi);
  for (int it = 0; it < SAC5_NEWTON; ++it) {
    const double xn = x - sac5_horner<D>(q, x) / sac5_horner<D - 1>(dq, x);
    if (xn > lo && xn < hi) x = xn;
  }
  *found = fa != fb;
  return x;
}

// One level of the root isolation: the polynomial of degree D of each team's chain on the intervals between the D + 1 points of
// the level below (pin), one interval per lane.  An interval without a sign change hands its left end on (an interval of width
// zero one level up: harmless).  Writes D + 2 points (pout) and the flags.
template <int D>
BA_HD void sac5_level(double* slab, int lane, int stride) {
  BA_NO_CONTRACT
  for (int l = lane; l < 64; l += stride) {
    const int team = l >> 5, i = l & 31;
    if (i >= D) continue;
    const double* qs = slab + SV_POLY + 66 * team + SV_OFF(D);
    const double* pin = slab + SV_PTS + 24 * team + 12 * (D & 1);
    double* pout = slab + SV_PTS + 24 * team + 12 * ((D + 1) & 1);
    const double a = pin[i];
    bool found;
    const double x = sac_interval_root<D>(qs, a, pin[i + 1], &found);
    pout[i + 1] = found ? x : a;
    slab[SV_FLAG + 12 * team + i] = found ? 1.0 : 0.0;
    if (i == 0) pout[0] = -1.0, pout[D + 1] = 1.0;
  }
  SOLVE_SYNC();
}

template <int D>
BA_HD void sac5_levels(double* slab, int lane, int stride) {
  if constexpr (D > 1) sac5_levels<D - 1>(slab, lane, stride);
  sac5_level<D>(slab, lane, stride);
}

// ---- five points: polish, decomposition, score --------------------------------------------------------------------------------------
BA_HD void sac5_mat33(const double* A, const double* B, double* C) {  // C = A B
  BA_NO_CONTRACT
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
BA_HD void sac5_mat33_nt(const double* A, const double* B, double* C) {  // C = A B^T
  BA_NO_CONTRACT
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1]) + A[3 * r + 2] * B[3 * c + 2];
}
BA_HD void sac5_mat33_tn(const double* A, const double* B, double* C) {  // C = A^T B
  BA_NO_CONTRACT
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[r] * B[c] + A[3 + r] * B[3 + c]) + A[6 + r] * B[6 + c];
}
BA_HD void sac5_cofactor(const double* E, double* K) {
  BA_NO_CONTRACT
  K[0] = E[4] * E[8] - E[5] * E[7], K[1] = E[5] * E[6] - E[3] * E[8], K[2] = E[3] * E[7] - E[4] * E[6];
  K[3] = E[7] * E[2] - E[8] * E[1], K[4] = E[8] * E[0] - E[6] * E[2], K[5] = E[6] * E[1] - E[7] * E[0];
  K[6] = E[1] * E[5] - E[2] * E[4], K[7] = E[2] * E[3] - E[0] * E[5], K[8] = E[0] * E[4] - E[1] * E[3];
}
BA_HD void sac5_essential(const double* B, const double* c, double* E) {
  BA_NO_CONTRACT
#pragma unroll
  for (int e = 0; e < 9; ++e) E[e] = ((c[0] * B[e] + c[1] * B[9 + e]) + c[2] * B[18 + e]) + c[3] * B[27 + e];
}
BA_HD void sac5_unit4(double* c) {
  BA_NO_CONTRACT
  const double n = sqrt(((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + c[3] * c[3]);
  c[0] = c[0] / n, c[1] = c[1] / n, c[2] = c[2] / n, c[3] = c[3] / n;
}

// One Gauss-Newton step on the ten cubics in the unit coefficient vector c of the null space basis B: residual r(c) (nine entries
// of E E^T E - 1/2 tr(E E^T) E, then det E), Jacobian J (10x4) by the product rule with dE = B_i, step (J^T J + c c^T) d = -J^T r
// (the second term pins the scale, along which r is homogeneous), c <- (c + d) / |c + d|.
BA_HD void sac5_polish_step(const double* B, double* c) {
  BA_NO_CONTRACT
  double E[9], H[9], G[9], K[9], res[10], J[40];
  sac5_essential(B, c, E);
  sac5_mat33_nt(E, E, H);
  sac5_mat33_tn(E, E, G);
  sac5_cofactor(E, K);
  const double half_tr = 0.5 * ((H[0] + H[4]) + H[8]);
  {
    double L[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) L[e] = H[e];
    L[0] = L[0] - half_tr, L[4] = L[4] - half_tr, L[8] = L[8] - half_tr;
    sac5_mat33(L, E, res);
    res[9] = (E[0] * K[0] + E[1] * K[1]) + E[2] * K[2];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double D[9], T1[9], T2[9], T3[9], M[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) D[e] = B[9 * i + e];
    sac5_mat33(D, G, T1);        // dE E^T E
    sac5_mat33_tn(D, E, M);      // dE^T E
    sac5_mat33(E, M, T2);        // E dE^T E
    sac5_mat33(H, D, T3);        // E E^T dE
    double tr = 0.0, dd = 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) tr = tr + E[e] * D[e], dd = dd + K[e] * D[e];
#pragma unroll
    for (int e = 0; e < 9; ++e) J[4 * e + i] = (((T1[e] + T2[e]) + T3[e]) - tr * E[e]) - half_tr * D[e];
    J[36 + i] = dd;
  }
  double N[16], g[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = c[i] * c[j];
#pragma unroll
      for (int e = 0; e < 10; ++e) s = s + J[4 * e + i] * J[4 * e + j];
      N[4 * i + j] = s;
    }
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < 10; ++e) s = s - J[4 * e + i] * res[e];
    g[i] = s;
  }
  // symmetric positive definite 4x4: elimination without pivoting
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int r = p + 1; r < 4; ++r) {
      const double f = N[4 * r + p] / N[4 * p + p];
#pragma unroll
      for (int k = p + 1; k < 4; ++k) N[4 * r + k] = N[4 * r + k] - f * N[4 * p + k];
      g[r] = g[r] - f * g[p];
    }
  double d[4];
#pragma unroll
  for (int p = 3; p >= 0; --p) {
    double s = g[p];
#pragma unroll
    for (int k = p + 1; k < 4; ++k) s = s - N[4 * p + k] * d[k];
    d[p] = s / N[4 * p + p];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = c[i] + d[i];
  sac5_unit4(c);
}

// the largest of the cross products of the three pairs of rows of a 3x3 (its null vector when the rank is two); w not normalised
BA_HD void sac5_null3(const double* A, double* w) {
  BA_NO_CONTRACT
  double x[3], best = -1.0;
  w[0] = w[1] = w[2] = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int r0 = a == 2 ? 1 : 0, r1 = a == 0 ? 1 : 2;  // (0,1), (0,2), (1,2)
    sac_cross(A + 3 * r0, A + 3 * r1, x);
    const double n = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    if (n > best) best = n, w[0] = x[0], w[1] = x[1], w[2] = x[2];
  }
}

// The coefficient vector c [4] of the root (zn : zd) of the polynomial, from the 3x3 polynomial matrix evaluated there in
// homogeneous form (so that |z| > 1 needs no division): (x zd, y zd, 1) spans its null space.
BA_HD void sac5_root_vector(const double* rows, double zn, double zd, double* c) {
  BA_NO_CONTRACT
  double A[9];
  const double n2 = zn * zn, d2 = zd * zd, n3 = n2 * zn, d3 = d2 * zd, n4 = n2 * n2, d4 = d2 * d2;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double* k = rows + 13 * r;
    A[3 * r] = ((k[0] * d3 + k[1] * (zn * d2)) + k[2] * (n2 * zd)) + k[3] * n3;
    A[3 * r + 1] = ((k[4] * d3 + k[5] * (zn * d2)) + k[6] * (n2 * zd)) + k[7] * n3;
    A[3 * r + 2] = (((k[8] * d4 + k[9] * (zn * d3)) + k[10] * (n2 * d2)) + k[11] * (n3 * zd)) + k[12] * n4;
  }
  double w[3];
  sac5_null3(A, w);
  c[0] = w[0], c[1] = w[1], c[2] = zn * w[2], c[3] = zd * w[2];
  sac5_unit4(c);
}

// the two ray parameters of sac_midpoint (fe_sac.hpp), with its arithmetic: the points l0 f1 and t12 + l1 R12 f2
BA_HD void sac_rays(const double* h, const double* f1, const double* f2, double* l0, double* l1) {
  BA_NO_CONTRACT
  const double* t = h + 12;
  double g[3];
  for (int k = 0; k < 3; ++k) g[k] = (h[k] * f2[0] + h[4 + k] * f2[1]) + h[8 + k] * f2[2];
  const double b0 = sac_dot3(t, f1), b1 = sac_dot3(t, g);
  const double a00 = sac_dot3(f1, f1), a10 = sac_dot3(f1, g), a01 = -a10, a11 = -sac_dot3(g, g);
  const double det = a00 * a11 - a01 * a10;
  *l0 = (a11 * b0 - a01 * b1) / det, *l1 = (a00 * b1 - a10 * b0) / det;
}

// Candidate `which` (bit 0: the rotation, bit 1: the sign of t) of the essential matrix E (unit Frobenius norm): its
// transformation T [12] (3x4 row-major, |t| = 1), and the sum of the eight scores, +inf unless all sixteen ray parameters are
// positive and everything is finite.  corr: [8][8].
BA_HD double sac5_candidate(const double* E, int which, const double* corr, double* T) {
  BA_NO_CONTRACT
  double Et[9], t[3], K[9], X[9], R[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Et[3 * r + c] = E[3 * c + r];
  sac5_null3(Et, t);  // t^T E = 0: orthogonal to the columns of E
  sac_unit(t);
  sac5_cofactor(E, K);
  const double X0[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};
  sac5_mat33(X0, E, X);
  const double s = (which & 1) ? sqrt(2.0) : -sqrt(2.0);
#pragma unroll
  for (int e = 0; e < 9; ++e) R[e] = 2.0 * K[e] + s * X[e];
  {  // one polar step R (3 I - R^T R) / 2: what the constraints' residual leaves of non-orthogonality is squared
    double Q[9], P[9];
    sac5_mat33_tn(R, R, Q);
#pragma unroll
    for (int e = 0; e < 9; ++e) Q[e] = -Q[e];
    Q[0] = 3.0 + Q[0], Q[4] = 3.0 + Q[4], Q[8] = 3.0 + Q[8];
    sac5_mat33(R, Q, P);
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = 0.5 * P[e];
  }
  const double sg = (which & 2) ? -1.0 : 1.0;
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    T[4 * r] = R[3 * r], T[4 * r + 1] = R[3 * r + 1], T[4 * r + 2] = R[3 * r + 2], T[4 * r + 3] = sg * t[r];
  }
#pragma unroll
  for (int e = 0; e < 12; ++e) ok = ok && sac_finite(T[e]);
  double h[SAC_MODEL_STRIDE];
  sac_stage_model(OKVIS_FE_SAC_RELATIVE, T, h);
  double sum = 0.0;
  for (int k = 0; k < 8; ++k) {
    const double* q = corr + 8 * k;
    double l0, l1;
    sac_rays(h, q, q + 3, &l0, &l1);
    ok = ok && l0 > 0.0 && l1 > 0.0;
    sum = sum + sac_score_relative(h, q, q + 3, q[6], q[7]);
  }
  return ok && sac_finite(sum) ? sum : __builtin_inf();
}

// ---- five points: one sample ----------------------------------------------------------------------------------------------------------
struct Sac5Out {
  double* model;       // [12], always written
  uint8_t* valid;      // or null
  int32_t* n_roots;    // or null
  double* essentials;  // [10][9] or null
};

// a, b: the bearing vectors of the two frames as [3][n]; s1, s2: sigmas or null; idx: the eight sample indices (in range).
BA_HD void sac5_wave(double* slab, int lane, int stride, const double* a, const double* b, size_t n, const double* s1,
                     const double* s2, const int32_t* idx, Sac5Out out) {
  BA_NO_CONTRACT
  bool bad = false;
  for (int i = 0; i < 8; ++i)
    for (int j = i + 1; j < 8; ++j) bad = bad || idx[i] == idx[j];
  int n_roots = 0, best = -1;
  if (!bad) {
    // the sample, and the columns of [A^T | I9]
    for (int l = lane; l < 8; l += stride) {
      const size_t k = (size_t)idx[l];
      double* q = slab + SV_CORR + 8 * l;
      for (int e = 0; e < 3; ++e) q[e] = a[e * n + k], q[3 + e] = b[e * n + k];
      q[6] = s1 ? s1[k] : 1.0, q[7] = s2 ? s2[k] : 1.0;
    }
    SOLVE_SYNC();
    double* M = slab + SV_MAT;
    for (int l = lane; l < 14; l += stride) {
      double* col = M + 9 * l;
      if (l < 5) {
        const double* q = slab + SV_CORR + 8 * l;
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) col[3 * r + c] = q[r] * q[3 + c];
      } else {
        for (int e = 0; e < 9; ++e) col[e] = e == l - 5 ? 1.0 : 0.0;
      }
    }
    SOLVE_SYNC();
#pragma unroll
    for (int k = 0; k < 5; ++k) {  // reflection k from column k, rows k..8; applied to the columns after it
      double v[9], nn = 0.0;
#pragma unroll
      for (int r = k; r < 9; ++r) v[r] = M[9 * k + r], nn = nn + v[r] * v[r];
      const double alpha = v[k] < 0.0 ? sqrt(nn) : -sqrt(nn);
      v[k] = v[k] - alpha;
      double vv = 0.0;
#pragma unroll
      for (int r = k; r < 9; ++r) vv = vv + v[r] * v[r];
      const double beta = 2.0 / vv;
      for (int l = lane + k + 1; l < 14; l += stride) {
        double* col = M + 9 * l;
        double s = 0.0;
#pragma unroll
        for (int r = k; r < 9; ++r) s = s + v[r] * col[r];
        const double f = s * beta;
#pragma unroll
        for (int r = k; r < 9; ++r) col[r] = col[r] - f * v[r];
      }
      SOLVE_SYNC();
    }
    double* B = slab + SV_B;
    for (int l = lane; l < 36; l += stride) {  // rows 5..8 of Q^T
      const int i = l / 9, e = l - 9 * i;
      B[l] = M[9 * (5 + e) + 5 + i];
    }
    SOLVE_SYNC();
    for (int l = lane; l < 10; l += stride) sac5_cubic(B, l, M + 20 * l);
    SOLVE_SYNC();
    for (int p = 0; p < 10; ++p) {
      int piv = p;
      double big = fabs(M[20 * p + p]);
      for (int r = p + 1; r < 10; ++r) {
        const double x = fabs(M[20 * r + p]);
        if (x > big) big = x, piv = r;
      }
      bad = bad || !(big > 0.0) || !sac_finite(big);
      if (piv != p) {
        for (int l = lane + p; l < 20; l += stride) {
          const double x = M[20 * p + l];
          M[20 * p + l] = M[20 * piv + l], M[20 * piv + l] = x;
        }
        SOLVE_SYNC();
      }
      for (int l = lane + p + 1; l < 20; l += stride) {  // column p itself is not read again
        const double pc = M[20 * p + l] / M[20 * p + p];
        M[20 * p + l] = pc;
        for (int r = 0; r < 10; ++r)
          if (r != p) M[20 * r + l] = M[20 * r + l] - M[20 * r + p] * pc;
      }
      SOLVE_SYNC();
    }
  }
  if (!bad) {
    const double* M = slab + SV_MAT;
    double* rows = slab + SV_ROWS;
    for (int l = lane; l < 3; l += stride) {  // <k> = <e> - z <f>, <l> = <g> - z <h>, <m> = <i> - z <j>
      const double *e = M + 20 * (4 + 2 * l) + 10, *f = M + 20 * (5 + 2 * l) + 10;
      double* k = rows + 13 * l;
      k[0] = e[2], k[1] = e[1] - f[2], k[2] = e[0] - f[1], k[3] = -f[0];
      k[4] = e[5], k[5] = e[4] - f[5], k[6] = e[3] - f[4], k[7] = -f[3];
      k[8] = e[9], k[9] = e[8] - f[9], k[10] = e[7] - f[8], k[11] = e[6] - f[7], k[12] = -f[6];
    }
    SOLVE_SYNC();
    double p[11];
    sac5_poly10(rows, p);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j <= 10; ++j) slab[SV_P + j] = p[j];
    }
    SOLVE_SYNC();
    // the derivative chains: team 0 of p, team 1 of the reversed polynomial; coefficient j of degree d is p[j + 10 - d] times
    // (j + 10 - d)! / j!
    for (int l = lane; l < 64; l += stride) {
      const int team = l >> 5, d = (l & 31) + 1;
      if (d > 10) continue;
      double* q = slab + SV_POLY + 66 * team + SV_OFF(d);
      for (int j = 0; j <= d; ++j) {
        const int s = j + 10 - d;
        double f = team ? slab[SV_P + 10 - s] : slab[SV_P + s];
        for (int m = 0; m < 10 - d; ++m) f = f * (double)(s - m);
        q[j] = f;
      }
      if (d == 1) {
        double* pts = slab + SV_PTS + 24 * team + 12;
        pts[0] = -1.0, pts[1] = 1.0;
      }
    }
    SOLVE_SYNC();
    sac5_levels<10>(slab, lane, stride);
    // level 10 left its points in buffer 1 and the flags; the roots in order: team 0 ascending, then team 1
    if (lane == 0) {
      int cnt = 0;
      for (int team = 0; team < 2; ++team)
        for (int i = 0; i < 10; ++i) {
          const double x = slab[SV_PTS + 24 * team + 12 + i + 1];
          const bool in = team == 0 ? true : (x > -1.0 && x < 1.0);  // |z| = 1 belongs to team 0
          if (slab[SV_FLAG + 12 * team + i] != 0.0 && in && cnt < SOLVE_MAX_ROOTS) slab[SV_SLOT + cnt++] = (double)(16 * team + i);
        }
      slab[SV_SLOT + 10] = (double)cnt;
    }
    SOLVE_SYNC();
    n_roots = (int)slab[SV_SLOT + 10];
    const double* B = slab + SV_B;
    for (int l = lane; l < n_roots; l += stride) {
      const int slot = (int)slab[SV_SLOT + l], team = slot >> 4, i = slot & 15;
      const double x = slab[SV_PTS + 24 * team + 12 + i + 1];
      double c[4], E[9];
      sac5_root_vector(rows, team ? 1.0 : x, team ? x : 1.0, c);
      for (int it = 0; it < SAC5_POLISH; ++it) sac5_polish_step(B, c);
      sac5_essential(B, c, E);
      const double nn = sqrt(((((((((E[0] * E[0] + E[1] * E[1]) + E[2] * E[2]) + E[3] * E[3]) + E[4] * E[4]) + E[5] * E[5]) + E[6] * E[6]) + E[7] * E[7]) + E[8] * E[8]));
#pragma unroll
      for (int e = 0; e < 9; ++e) slab[SV_E + 9 * l + e] = E[e] / nn;
#pragma unroll
      for (int e = 0; e < 4; ++e) slab[SV_C + 4 * l + e] = c[e];
    }
    SOLVE_SYNC();
    for (int l = lane; l < 4 * n_roots; l += stride) {
      double T[12];
      slab[SV_SUM + l] = sac5_candidate(slab + SV_E + 9 * (l >> 2), l & 3, slab + SV_CORR, T);
#pragma unroll
      for (int e = 0; e < 12; ++e) slab[SV_CAND + 12 * l + e] = T[e];
    }
    SOLVE_SYNC();
    double least = __builtin_inf();
    for (int l = 0; l < 4 * n_roots; ++l) {
      const double s = slab[SV_SUM + l];
      if (s < least) least = s, best = l;
    }
  }
  for (int l = lane; l < 12; l += stride) out.model[l] = best >= 0 ? slab[SV_CAND + 12 * best + l] : sac_nan();
  if (lane == 0) {
    if (out.valid) *out.valid = best >= 0 ? 1 : 0;
    if (out.n_roots) *out.n_roots = n_roots;
  }
  if (out.essentials)
    for (int l = lane; l < 9 * n_roots; l += stride) out.essentials[l] = slab[SV_E + l];
  SOLVE_SYNC();  // the slab is free for the next sample (host loops reuse it)
}

#if defined(__HIPCC__)
struct SolveJob {  // one job of okvis_fe_sac_solve, device pointers
  const double *a, *b;        // [3][n]
  const double *sigma1, *sigma2;  // [n] or null
  const int32_t* samples;     // [n_models][2 or 8]
  double* models;             // [n_models][9 or 12]
  uint8_t* valid;             // [n_models] or null
  int32_t* n_roots;           // [n_models] or null
  double* essentials;         // [n_models][10][9] or null
  int32_t kind, n, n_models;
  int32_t block0;             // first workgroup of the job in the grid
};

struct SolveParams {
  const SolveJob* jobs;
  int32_t n_jobs;
};

// One wave per workgroup.  A relative job takes one workgroup per sample, a rotation-only job one per 64 samples.
__global__ __launch_bounds__(64) void sac_solve_kernel(SolveParams P) {
  __shared__ double slab[SOLVE_SLAB];
  const SolveJob J = P.jobs[find_job(P.jobs, P.n_jobs, &SolveJob::block0)];
  const int local = (int)blockIdx.x - J.block0, lane = threadIdx.x;
  const size_t n = (size_t)J.n;
  if (J.kind == OKVIS_FE_SAC_ROTATION_ONLY) {
    const int m = local * 64 + lane;
    if (m >= J.n_models) return;
    const size_t i = (size_t)J.samples[2 * m], j = (size_t)J.samples[2 * m + 1];
    const double f1i[3] = {J.a[i], J.a[n + i], J.a[2 * n + i]}, f1j[3] = {J.a[j], J.a[n + j], J.a[2 * n + j]};
    const double f2i[3] = {J.b[i], J.b[n + i], J.b[2 * n + i]}, f2j[3] = {J.b[j], J.b[n + j], J.b[2 * n + j]};
    double R[9];
    const bool ok = i != j && sac2_rotation(f1i, f1j, f2i, f2j, R);
#pragma unroll
    for (int e = 0; e < 9; ++e) J.models[9 * (size_t)m + e] = ok ? R[e] : sac_nan();
    if (J.valid) J.valid[m] = ok ? 1 : 0;
    return;
  }
  Sac5Out out;
  out.model = J.models + 12 * (size_t)local;
  out.valid = J.valid ? J.valid + local : nullptr;
  out.n_roots = J.n_roots ? J.n_roots + local : nullptr;
  out.essentials = J.essentials ? J.essentials + 90 * (size_t)local : nullptr;
  sac5_wave(slab, lane, 64, J.a, J.b, n, J.sigma1, J.sigma2, J.samples + 8 * (size_t)local, out);
}
#endif  // __HIPCC__

}  // namespace fe
