// The minimal solver of Frontend::runRansac3d2d (okvis_frontend/src/Frontend.cpp:575-642) on the device
// (include/okvis_amd_frontend.h: okvis_fe_sac_solve_absolute): a pose of the body from three correspondences between world points
// and bearing vectors of several cameras, plus a fourth that picks the pose (FrameAbsolutePoseSacProblem, Algorithm::GP3P).  The
// solver is OpenGV's generated Groebner-basis code and OpenGV's source is not part of the reference tree: it is stated from its
// mathematical definition and is NOT pinned to OpenGV ("3D-2D hypotheses").
//
// Convention (the consensus entry's): a hypothesis (R, t) takes a body point to the world, X = R p + t.
//
// Definition.  Correspondence k = 0..2 of the sample: c_k its camera's offset, d_k = (its camera's rotation) (its bearing), X_k
// its world point.  The candidates are all real (l0, l1, l2), every l_k > 0, with
//     |(c_a + l_a d_a) - (c_b + l_b d_b)|^2 = |X_a - X_b|^2      for (a, b) = (0, 1), (0, 2), (1, 2):
// three quadrics, at most eight solutions.  With p_k = c_k + l_k d_k the candidate is the rigid transformation that takes the p_k to
// the X_k: R = a1 b1^T + a2 b2^T + a3 b3^T from the frames (a1, a2, a3) = (u / |u|, (a1 x v) / |.|, a1 x a2), u = X_1 - X_0,
// v = X_2 - X_0, and (b1, b2, b3) alike from the p_k (the two-point solver's frames: sac2_frame), t = X_0 - R p_0.  The hypothesis
// is the candidate with the smallest |reprojection - bearing|^2 of the fourth correspondence (sac_score_absolute with sigma = 1).
// Invalid: two equal indices, |u x v| zero or not finite, no candidate.  One camera (the central problem) is the same definition
// through the same code.
//
// Route (gp3_group):
//   1  the three quadrics' coefficients (gp3_quadric)
//   2  the resultant in l0 of the two quadrics that hold it, a quartic G(l1, l2); G modulo the third quadric (quadratic in l2) is
//      A(l1) + B(l1) l2; the third quadric at l2 = -A / B times B^2 is the octic in l1 (gp3_octic)
//   3  its positive roots: p on [0, 1] and the reversed polynomial on [0, 1] for l1 > 1 (two teams of lanes), that is, all of
//      l1 > 0 with no bound assumed on the scene.  The derivative chain of fe_sac_solve.hpp at degree eight (sac_interval_root):
//      every loop has a compile-time count
//   4  per root: l0 and l2 from the two quadrics that are quadratic in them at this l1 (of the four pairs the one that fits the
//      third best), then GP3_POLISH Newton steps on the three quadrics themselves in their geometric form, 3 x 3, so that what is
//      left is the rounding of the definition and not of steps 2 and 3
//   5  per root: accepted when finite, all depths positive and the quadrics hold; the frames, the transformation, the fourth
//      correspondence's score
//   6  the accepted candidate with the smallest score
// No workgroup barrier, no atomics, all fp64.  GP3_GROUP = 16 lanes per sample (eight intervals of two teams at the last level,
// one root per lane after it), four samples per wave, each with its own LDS slab of GP3_SLAB doubles.
//
// gp3_group is ONE source for the device and the host, like sac5_wave: the device calls it with (lane in the group, 16), a plain
// host compiler with (0, 1).  Code outside the "lanes take ..." loops is uniform over the group.
#pragma once
#include "fe_sac_solve.hpp"

namespace fe {

constexpr int GP3_GROUP = 16;                    // lanes per sample
constexpr int GP3_PER_WAVE = 64 / GP3_GROUP;     // samples per wave = per workgroup
constexpr int GP3_POLISH = 4;                    // Newton steps on the definition
constexpr int GP3_MAX_ROOTS = OKVIS_FE_SAC_MAX_ROOTS_ABSOLUTE;
constexpr double GP3_RESIDUAL = 1e-9;            // a candidate's quadrics hold to this part of their terms (a polished root: 1e-15)

// the sample's slab, offsets in doubles
constexpr int GS_C = 0;        // [3][3] camera offsets
constexpr int GS_D = 9;        // [3][3] ray directions in the body
constexpr int GS_X = 18;       // [3][3] world points
constexpr int GS_F = 27;       // the fourth correspondence: world point (3), bearing (3), camera (12)
constexpr int GS_Q = 45;       // [3][6] the quadrics (0,1), (0,2), (1,2): la^2, lb^2, la lb, la, lb, 1
constexpr int GS_P = 63;       // [9] the octic, ascending
constexpr int GS_POLY = 72;    // [2][45] per team the derivative chain: degree d at SV_OFF(d)
constexpr int GS_PTS = 162;    // [2][2][10] per team two buffers of interval ends
constexpr int GS_FLAG = 202;   // [2][10] per team: interval i of the last level holds a root
constexpr int GS_SLOT = 222;   // [8] team * 8 + interval of root r; [8] the number of roots; then [8] the accepted roots in order
constexpr int GS_CAND = 240;   // [8][12] the roots' transformations
constexpr int GS_SCORE = 336;  // [8] their scores, +inf for a root that is not accepted
constexpr int GP3_SLAB = 344;

// the quadric of the pair (a, b) in (la, lb): |(ca + la da) - (cb + lb db)|^2 - |Xa - Xb|^2
BA_HD void gp3_quadric(const double* ca, const double* da, const double* Xa, const double* cb, const double* db, const double* Xb, double* q) {
  BA_NO_CONTRACT
  const double w[3] = {ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2]};
  q[0] = sac_dot3(da, da), q[1] = sac_dot3(db, db), q[2] = -2.0 * sac_dot3(da, db);
  q[3] = 2.0 * sac_dot3(da, w), q[4] = -2.0 * sac_dot3(db, w), q[5] = sac_dot3(w, w) - sac_sqdist(Xa, Xb);
}

// out (+)= sgn * a * b for polynomials in (x, y) kept as [5][5] (x^i y^j at 5 i + j), a of degree (AX, AY), b of (BX, BY)
template <int AX, int AY, int BX, int BY>
BA_HD void gp3_bimul(const double* a, const double* b, double sgn, double* out) {
  BA_NO_CONTRACT
#pragma unroll
  for (int i = 0; i <= AX; ++i)
#pragma unroll
    for (int j = 0; j <= AY; ++j)
#pragma unroll
      for (int k = 0; k <= BX; ++k)
#pragma unroll
        for (int l = 0; l <= BY; ++l) out[5 * (i + k) + j + l] = out[5 * (i + k) + j + l] + sgn * (a[5 * i + j] * b[5 * k + l]);
}

// q: the three quadrics [3][6]; P[9]: the octic in l1, ascending
BA_HD void gp3_octic(const double* q, double* P) {
  BA_NO_CONTRACT
  const double *q01 = q, *q02 = q + 6, *q12 = q + 12;
  // in l0: (0,1) is a t^2 + (b0 + b1 x) t + (c0 + c1 x + c2 x^2), (0,2) is a' t^2 + (b'0 + b'1 y) t + (c'0 + c'1 y + c'2 y^2)
  const double a = q01[0], b0 = q01[3], b1 = q01[2], c0 = q01[5], c1 = q01[4], c2 = q01[1];
  const double a_ = q02[0], b0_ = q02[3], b1_ = q02[2], c0_ = q02[5], c1_ = q02[4], c2_ = q02[1];
  double u[25], v[25], z[25], G[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) u[i] = 0.0, v[i] = 0.0, z[i] = 0.0, G[i] = 0.0;
  u[0] = a * c0_ - a_ * c0, u[1] = a * c1_, u[2] = a * c2_, u[5] = -(a_ * c1), u[10] = -(a_ * c2);   // a c' - a' c
  v[0] = a * b0_ - a_ * b0, v[1] = a * b1_, v[5] = -(a_ * b1);                                         // a b' - a' b
  z[0] = b0 * c0_ - b0_ * c0, z[1] = b0 * c1_ - b1_ * c0, z[2] = b0 * c2_;                              // b c' - b' c
  z[5] = b1 * c0_ - b0_ * c1, z[6] = b1 * c1_ - b1_ * c1, z[7] = b1 * c2_;
  z[10] = -(b0_ * c2), z[11] = -(b1_ * c2);
  gp3_bimul<2, 2, 2, 2>(u, u, 1.0, G);   // the resultant: (a c' - a' c)^2 - (a b' - a' b)(b c' - b' c)
  gp3_bimul<1, 1, 2, 2>(v, z, -1.0, G);
  double g0[5], g1[4], g2[3], g3[2], g4[1];
#pragma unroll
  for (int i = 0; i < 5; ++i) g0[i] = G[5 * i];
#pragma unroll
  for (int i = 0; i < 4; ++i) g1[i] = G[5 * i + 1];
#pragma unroll
  for (int i = 0; i < 3; ++i) g2[i] = G[5 * i + 2];
#pragma unroll
  for (int i = 0; i < 2; ++i) g3[i] = G[5 * i + 3];
  g4[0] = G[4];
  // (1,2) in l2: e y^2 + l(x) y + k(x); y^2 = m1 y + m0
  const double e = q12[1], l[2] = {q12[4], q12[2]}, k[3] = {q12[5], q12[3], q12[0]};
  const double m1[2] = {-l[0] / e, -l[1] / e}, m0[3] = {-k[0] / e, -k[1] / e, -k[2] / e};
  double s[3] = {m0[0], m0[1], m0[2]}, m1m0[4] = {0.0, 0.0, 0.0, 0.0};
  sac5_polymul<2, 2>(m1, m1, 1.0, s);        // y^3 = s y + m1 m0
  sac5_polymul<2, 3>(m1, m0, 1.0, m1m0);
  double t3[4] = {m1m0[0], m1m0[1], m1m0[2], m1m0[3]}, t4[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  sac5_polymul<3, 2>(s, m1, 1.0, t3);        // y^4 = t3 y + t4
  sac5_polymul<3, 3>(s, m0, 1.0, t4);
  double A[5] = {g0[0], g0[1], g0[2], g0[3], g0[4]}, B[4] = {g1[0], g1[1], g1[2], g1[3]};
  sac5_polymul<3, 3>(g2, m0, 1.0, A);
  sac5_polymul<2, 4>(g3, m1m0, 1.0, A);
  sac5_polymul<1, 5>(g4, t4, 1.0, A);
  sac5_polymul<3, 2>(g2, m1, 1.0, B);
  sac5_polymul<2, 3>(g3, s, 1.0, B);
  sac5_polymul<1, 4>(g4, t3, 1.0, B);
  double AA[9], AB[8], BB[7], eA[1] = {e};
#pragma unroll
  for (int i = 0; i < 9; ++i) AA[i] = 0.0, P[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) AB[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 7; ++i) BB[i] = 0.0;
  sac5_polymul<5, 5>(A, A, 1.0, AA);
  sac5_polymul<5, 4>(A, B, 1.0, AB);
  sac5_polymul<4, 4>(B, B, 1.0, BB);
  sac5_polymul<1, 9>(eA, AA, 1.0, P);        // e A^2 - l A B + k B^2
  sac5_polymul<2, 8>(l, AB, -1.0, P);
  sac5_polymul<3, 7>(k, BB, 1.0, P);
}

// One level of the root isolation on [0, 1], as sac5_level: team = l >> 3, interval = l & 7
template <int D>
BA_HD void gp3_level(double* slab, int lane, int stride) {
  for (int l = lane; l < GP3_GROUP; l += stride) {
    const int team = l >> 3, i = l & 7;
    if (i >= D) continue;
    const double* pin = slab + GS_PTS + 20 * team + 10 * (D & 1);
    double* pout = slab + GS_PTS + 20 * team + 10 * ((D + 1) & 1);
    const double a = pin[i];
    bool found;
    const double x = sac_interval_root<D>(slab + GS_POLY + 45 * team + SV_OFF(D), a, pin[i + 1], &found);
    pout[i + 1] = found ? x : a;
    slab[GS_FLAG + 10 * team + i] = found ? 1.0 : 0.0;
    if (i == 0) pout[0] = 0.0, pout[D + 1] = 1.0;
  }
  SOLVE_SYNC();
}

template <int D>
BA_HD void gp3_levels(double* slab, int lane, int stride) {
  if constexpr (D > 1) gp3_levels<D - 1>(slab, lane, stride);
  gp3_level<D>(slab, lane, stride);
}

// the two roots of a t^2 + b t + c, a negative discriminant (a rounded double root) taken as zero
BA_HD void gp3_quadratic(double a, double b, double c, double* t) {
  BA_NO_CONTRACT
  double disc = b * b - 4.0 * (a * c);
  if (disc < 0.0) disc = 0.0;
  const double r = sqrt(disc);
  t[0] = (-b - r) / (2.0 * a), t[1] = (-b + r) / (2.0 * a);
}

// the three quadrics at the depths lam in their geometric form: F [3], and per pair r . da and r . db (r = pa - pb) in g [3][2];
// the largest of |r|^2 + |Xa - Xb|^2 in *size
BA_HD void gp3_residual(const double* slab, const double* lam, double* F, double* g, double* size) {
  BA_NO_CONTRACT
  double p[9];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int e = 0; e < 3; ++e) p[3 * k + e] = slab[GS_C + 3 * k + e] + lam[k] * slab[GS_D + 3 * k + e];
  double big = 0.0;
#pragma unroll
  for (int pair = 0; pair < 3; ++pair) {
    const int a = pair == 2 ? 1 : 0, b = pair == 0 ? 1 : 2;
    const double r[3] = {p[3 * a] - p[3 * b], p[3 * a + 1] - p[3 * b + 1], p[3 * a + 2] - p[3 * b + 2]};
    const double rr = sac_dot3(r, r), D = sac_sqdist(slab + GS_X + 3 * a, slab + GS_X + 3 * b);
    F[pair] = rr - D;
    g[2 * pair] = sac_dot3(r, slab + GS_D + 3 * a), g[2 * pair + 1] = sac_dot3(r, slab + GS_D + 3 * b);
    if (rr + D > big) big = rr + D;
  }
  *size = big;
}

// The candidate of the root x of the octic (l1): its transformation T [12] (3x4 row-major) and the fourth correspondence's score;
// +inf (T untouched or not) for a root that is not accepted
BA_HD double gp3_candidate(const double* slab, double x, double* T) {
  BA_NO_CONTRACT
  const double *q01 = slab + GS_Q, *q02 = q01 + 6, *q12 = q01 + 12;
  double t[2], y[2];
  gp3_quadratic(q01[0], q01[2] * x + q01[3], (q01[1] * x + q01[4]) * x + q01[5], t);
  gp3_quadratic(q12[1], q12[2] * x + q12[4], (q12[0] * x + q12[3]) * x + q12[5], y);
  double lam[3] = {t[0], x, y[0]}, least = 0.0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const double tt = t[w & 1], yy = y[w >> 1];
    const double f = fabs(((((q02[0] * tt) * tt + (q02[1] * yy) * yy) + (q02[2] * tt) * yy) + (q02[3] * tt + q02[4] * yy)) + q02[5]);
    if (w == 0 || f < least) least = f, lam[0] = tt, lam[2] = yy;
  }
  double F[3], g[6], size;
  for (int it = 0; it < GP3_POLISH; ++it) {
    gp3_residual(slab, lam, F, g, &size);
    // J = 2 [g0 -g1 0; g2 0 -g3; 0 g4 -g5], J delta = -F by Cramer's rule
    const double j00 = 2.0 * g[0], j01 = -2.0 * g[1], j10 = 2.0 * g[2], j12 = -2.0 * g[3], j21 = 2.0 * g[4], j22 = -2.0 * g[5];
    const double n0 = -F[0], n1 = -F[1], n2 = -F[2];
    const double det = -((j00 * j12) * j21) - (j01 * j10) * j22;
    const double h = n1 * j22 - j12 * n2;
    const double d0 = -((n0 * j12) * j21) - j01 * h;
    const double d1 = j00 * h - n0 * (j10 * j22);
    const double d2 = (-((j00 * n1) * j21) - (j01 * j10) * n2) + n0 * (j10 * j21);
    lam[0] = lam[0] + d0 / det, lam[1] = lam[1] + d1 / det, lam[2] = lam[2] + d2 / det;
  }
  gp3_residual(slab, lam, F, g, &size);
  bool ok = lam[0] > 0.0 && lam[1] > 0.0 && lam[2] > 0.0 && sac_finite(lam[0]) && sac_finite(lam[1]) && sac_finite(lam[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) ok = ok && fabs(F[k]) <= GP3_RESIDUAL * size;
  if (!ok) return __builtin_inf();
  double p[9];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int e = 0; e < 3; ++e) p[3 * k + e] = slab[GS_C + 3 * k + e] + lam[k] * slab[GS_D + 3 * k + e];
  const double* X = slab + GS_X;
  double a1[3] = {X[3] - X[0], X[4] - X[1], X[5] - X[2]}, b1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]};
  const double av[3] = {X[6] - X[0], X[7] - X[1], X[8] - X[2]}, bv[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
  sac_unit(a1);
  sac_unit(b1);
  double a2[3], a3[3], b2[3], b3[3];
  if (!sac2_frame(a1, av, a2, a3) || !sac2_frame(b1, bv, b2, b3)) return __builtin_inf();
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) T[4 * r + c] = (a1[r] * b1[c] + a2[r] * b2[c]) + a3[r] * b3[c];
    T[4 * r + 3] = X[r] - ((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]);
  }
#pragma unroll
  for (int e = 0; e < 12; ++e) ok = ok && sac_finite(T[e]);
  double h[SAC_MODEL_STRIDE];
  sac_stage_model(OKVIS_FE_SAC_ABSOLUTE, T, h);
  const double s = sac_score_absolute(h, slab + GS_F, slab + GS_F + 3, 1.0, slab + GS_F + 6);
  return ok && sac_finite(s) ? s : __builtin_inf();
}

struct Gp3Out {
  double* model;       // [12], always written
  uint8_t* valid;      // or null
  int32_t* n_roots;    // or null
  double* candidates;  // [8][12] or null: all 96 written, NaN past n_roots
};

// pts, brg: world points and bearing vectors as [3][n]; cam_index [n] (in range); cams [n_cams][12]: offset (3), rotation (9,
// row-major); idx: the four sample indices (in range).
BA_HD void gp3_group(double* slab, int lane, int stride, const double* pts, const double* brg, size_t n, const int32_t* cam_index,
                     const double* cams, const int32_t* idx, Gp3Out out) {
  BA_NO_CONTRACT
  bool bad = false;
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j) bad = bad || idx[i] == idx[j];
  int n_roots = 0, best = -1;
  if (!bad) {
    for (int l = lane; l < 4; l += stride) {
      const size_t k = (size_t)idx[l];
      const double* cam = cams + 12 * (size_t)cam_index[k];
      const double f[3] = {brg[k], brg[n + k], brg[2 * n + k]};
      if (l < 3) {
        for (int e = 0; e < 3; ++e) {
          slab[GS_C + 3 * l + e] = cam[e], slab[GS_X + 3 * l + e] = pts[e * n + k];
          slab[GS_D + 3 * l + e] = (cam[3 + 3 * e] * f[0] + cam[4 + 3 * e] * f[1]) + cam[5 + 3 * e] * f[2];
        }
      } else {
        for (int e = 0; e < 3; ++e) slab[GS_F + e] = pts[e * n + k], slab[GS_F + 3 + e] = f[e];
        for (int e = 0; e < 12; ++e) slab[GS_F + 6 + e] = cam[e];
      }
    }
    SOLVE_SYNC();
    const double* X = slab + GS_X;
    const double u[3] = {X[3] - X[0], X[4] - X[1], X[5] - X[2]}, v[3] = {X[6] - X[0], X[7] - X[1], X[8] - X[2]};
    double w[3];
    sac_cross(u, v, w);
    const double nn = sqrt(sac_dot3(w, w));
    bad = !(nn > 0.0) || !sac_finite(nn);
  }
  if (!bad) {
    double q[18], P[9];
#pragma unroll
    for (int pair = 0; pair < 3; ++pair) {
      const int a = pair == 2 ? 1 : 0, b = pair == 0 ? 1 : 2;
      gp3_quadric(slab + GS_C + 3 * a, slab + GS_D + 3 * a, slab + GS_X + 3 * a, slab + GS_C + 3 * b, slab + GS_D + 3 * b, slab + GS_X + 3 * b,
                  q + 6 * pair);
    }
    gp3_octic(q, P);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 18; ++j) slab[GS_Q + j] = q[j];
#pragma unroll
      for (int j = 0; j <= 8; ++j) slab[GS_P + j] = P[j];
    }
    SOLVE_SYNC();
    // the derivative chains: team 0 of p, team 1 of the reversed polynomial; coefficient j of degree d is p[j + 8 - d] times
    // (j + 8 - d)! / j!
    for (int l = lane; l < GP3_GROUP; l += stride) {
      const int team = l >> 3, d = (l & 7) + 1;
      double* c = slab + GS_POLY + 45 * team + SV_OFF(d);
      for (int j = 0; j <= d; ++j) {
        const int s = j + 8 - d;
        double f = team ? slab[GS_P + 8 - s] : slab[GS_P + s];
        for (int m = 0; m < 8 - d; ++m) f = f * (double)(s - m);
        c[j] = f;
      }
      if (d == 1) {
        double* ends = slab + GS_PTS + 20 * team + 10;
        ends[0] = 0.0, ends[1] = 1.0;
      }
    }
    SOLVE_SYNC();
    gp3_levels<8>(slab, lane, stride);
    // level 8 left its points in buffer 1 and the flags; the roots in order: team 0 ascending (l1 in (0, 1]), then team 1
    // (1 / l1 in (0, 1), descending l1)
    if (lane == 0) {
      int cnt = 0;
      for (int team = 0; team < 2; ++team)
        for (int i = 0; i < 8; ++i) {
          const double x = slab[GS_PTS + 20 * team + 10 + i + 1];
          const bool in = team == 0 ? x > 0.0 : (x > 0.0 && x < 1.0);   // l1 = 1 belongs to team 0
          if (slab[GS_FLAG + 10 * team + i] != 0.0 && in && cnt < GP3_MAX_ROOTS) slab[GS_SLOT + cnt++] = (double)(8 * team + i);
        }
      slab[GS_SLOT + 8] = (double)cnt;
    }
    SOLVE_SYNC();
    const int found = (int)slab[GS_SLOT + 8];
    for (int l = lane; l < found; l += stride) {
      const int slot = (int)slab[GS_SLOT + l], team = slot >> 3, i = slot & 7;
      const double x = slab[GS_PTS + 20 * team + 10 + i + 1];
      double T[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) T[e] = sac_nan();
      slab[GS_SCORE + l] = gp3_candidate(slab, team ? 1.0 / x : x, T);
#pragma unroll
      for (int e = 0; e < 12; ++e) slab[GS_CAND + 12 * l + e] = T[e];
    }
    SOLVE_SYNC();
    double least = __builtin_inf();
    for (int l = 0; l < found; ++l) {
      const double s = slab[GS_SCORE + l];
      if (s < __builtin_inf()) {
        if (lane == 0) slab[GS_SLOT + 9 + n_roots] = (double)l;
        ++n_roots;
      }
      if (s < least) least = s, best = l;
    }
    SOLVE_SYNC();
  }
  for (int l = lane; l < 12; l += stride) out.model[l] = best >= 0 ? slab[GS_CAND + 12 * best + l] : sac_nan();
  if (lane == 0) {
    if (out.valid) *out.valid = best >= 0 ? 1 : 0;
    if (out.n_roots) *out.n_roots = n_roots;
  }
  if (out.candidates)
    for (int l = lane; l < 12 * GP3_MAX_ROOTS; l += stride) {
      const int r = l / 12;
      out.candidates[l] = r < n_roots ? slab[GS_CAND + 12 * (int)slab[GS_SLOT + 9 + r] + (l - 12 * r)] : sac_nan();
    }
  SOLVE_SYNC();  // the slab is free for the next sample (host loops reuse it)
}

#if defined(__HIPCC__)
struct Gp3Job {  // one job of okvis_fe_sac_solve_absolute, device pointers
  const double *points, *bearing;  // [3][n]
  const int32_t* cam_index;        // [n]
  const double* cams;              // [n_cams][12]
  const int32_t* samples;          // [n_models][4]
  double* models;                  // [n_models][12]
  uint8_t* valid;                  // [n_models] or null
  int32_t* n_roots;                // [n_models] or null
  double* candidates;              // [n_models][8][12] or null
  int32_t n, n_models;
  int32_t block0;                  // first workgroup of the job in the grid
};

struct Gp3Params {
  const Gp3Job* jobs;
  int32_t n_jobs;
};

// One wave per workgroup, GP3_PER_WAVE samples of one job per wave.
__global__ __launch_bounds__(64) void sac_gp3p_kernel(Gp3Params P) {
  __shared__ double slabs[GP3_PER_WAVE * GP3_SLAB];
  const Gp3Job J = P.jobs[find_job(P.jobs, P.n_jobs, &Gp3Job::block0)];
  const int group = threadIdx.x / GP3_GROUP, lane = threadIdx.x % GP3_GROUP;
  const int m = ((int)blockIdx.x - J.block0) * GP3_PER_WAVE + group;
  if (m >= J.n_models) return;
  Gp3Out out;
  out.model = J.models + 12 * (size_t)m;
  out.valid = J.valid ? J.valid + m : nullptr;
  out.n_roots = J.n_roots ? J.n_roots + m : nullptr;
  out.candidates = J.candidates ? J.candidates + 12 * GP3_MAX_ROOTS * (size_t)m : nullptr;
  gp3_group(slabs + GP3_SLAB * group, lane, GP3_GROUP, J.points, J.bearing, (size_t)J.n, J.cam_index, J.cams, J.samples + 4 * (size_t)m, out);
}
#endif  // __HIPCC__

}  // namespace fe
