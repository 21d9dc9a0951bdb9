// Outlier rejection of the OKVIS frontend on the device (include/okvis_amd_frontend.h: okvis_fe_bearing_vectors,
// okvis_fe_sac_consensus): what Frontend::runRansac3d2d / runRansac2d2d (okvis_frontend/src/Frontend.cpp:575-642, 645-810) compute
// per (hypothesis, correspondence) cell, for all cells of many problems in one launch.
//
// Restated from the reference:
//   bearing_vectors_kernel   the per-keypoint part of both adapters' constructors: backProject, normalize(), sigmaAngle
//                            (okvis_frontend/src/FrameNoncentralAbsoluteAdapter.cpp:96-149, FrameRelativeAdapter.cpp:168-244)
//   sac_score_absolute       FrameAbsolutePoseSacProblem::getSelectedDistancesToModel
//                            (okvis_frontend/include/opengv/sac_problems/absolute_pose/FrameAbsolutePoseSacProblem.hpp:129-161)
//   sac_score_rotation_only  FrameRotationOnlySacProblem::getSelectedDistancesToModel (.../relative_pose/FrameRotationOnlySacProblem.hpp:122-144)
//   sac_score_relative       FrameRelativePoseSacProblem::getSelectedDistancesToModel (.../relative_pose/FrameRelativePoseSacProblem.hpp:126-161)
//   sac_midpoint             opengv::triangulation::triangulate2, which the relative-pose score calls.  OpenGV's source is not part of
//                            the reference tree: this is the published two-view midpoint method (the closest points of the two rays
//                            under (R12, t12), then their mean), NOT pinned to reference lines.
// The scores are differences of unit vectors, squared, over a sigma of about 1e-6: every product and sum is rounded on its own and
// in the reference's order (BA_NO_CONTRACT, like ba_math.hpp's qmul_strict), so that no fused multiply-add forms across the
// error = reprojection - bearing cancellation.
//
// sac_consensus_kernel: one grid for all jobs of a call.  A workgroup takes SAC_THREADS correspondences of one job and up to
// SAC_MODEL_TILE of its hypotheses (few: the grid is small and the walk is latency); the hypotheses (with their inverses, formed once per hypothesis as the reference does) sit in
// LDS and are read as broadcasts, the correspondences are read once, coalesced from SoA arrays, and stay in registers.  Each lane
// owns one correspondence and walks the hypotheses; per (hypothesis, 64 correspondences) the wave writes its ballot word and adds
// the word's popcount to the hypothesis's count with one integer atomic: order-independent, deterministic.
//
// The score functions are BA_HD like ba_math.hpp's: a plain host compiler sees them too (tools/sac_cpu_loop.cpp times the same
// formulas on one core); the kernels are for hipcc only.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/okvis_amd_frontend.h"
#include "ba_math.hpp"
#if defined(__HIPCC__)
#include "fe_kernels.hpp"
#endif

namespace fe {

constexpr int SAC_THREADS = 256;     // correspondences per workgroup, one per lane
constexpr int SAC_WAVES = SAC_THREADS / 64;
constexpr int SAC_MODEL_TILE = 8;    // hypotheses in LDS per workgroup: a lane's walk is a dependent chain of fp64 divisions and
                                     // square roots (about 1 us per relative-pose hypothesis), so a short walk and more workgroups
constexpr int SAC_MODEL_STRIDE = 16; // doubles per staged hypothesis
constexpr int SAC_MAX_MODELS = 1024;
constexpr int SAC_MAX_N = 65536;
constexpr int SAC_MAX_CAMS = 8;

#if defined(__HIPCC__)
struct BearingParams {
  Camera cam;
  int n;
  const float* kp;   // [n][3]
  double* bearing;   // [n][3]
  double* sigma;     // [n]
  uint8_t* ok;       // [n]
};

struct SacJob {  // one problem of okvis_fe_sac_consensus, device pointers
  const double* models;      // [n_models][12] (3x4 row-major) or [n_models][9]
  const double* a;           // [3][n]: world points (absolute) or bearing vectors of frame 1
  const double* b;           // [3][n]: bearing vectors (absolute) or bearing vectors of frame 2
  const double* sigma1;      // [n]
  const double* sigma2;      // [n], the relative kinds
  const int32_t* cam_index;  // [n], absolute
  const double* cams;        // [n_cams][12]: offset (3), rotation (9, row-major), absolute
  double* scores;            // [n_models][n] or null
  double threshold;
  int32_t kind, n, n_models;
  int32_t block0;            // first workgroup of the job in the grid
  int32_t tiles;             // ceil(n / SAC_THREADS)
  int32_t count0;            // first entry of the job in counts
  int64_t word0;             // first ballot word of the job: ballots[word0 + m * ceil(n / 64) + w]
};

struct SacParams {
  const SacJob* jobs;
  int32_t n_jobs;
  int32_t* counts;                 // zero on entry
  unsigned long long* ballots;
};

__global__ __launch_bounds__(256) void bearing_vectors_kernel(BearingParams P) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.n) return;
  const float* kp = P.kp + 3 * (size_t)i;
  double dir[3];
  const bool ok = back_project(P.cam, (double)kp[0], (double)kp[1], dir);
  normalize3(dir);
  if (P.bearing) P.bearing[3 * (size_t)i] = dir[0], P.bearing[3 * (size_t)i + 1] = dir[1], P.bearing[3 * (size_t)i + 2] = dir[2];
  if (P.sigma) {
    const double sd = 0.8 * (double)kp[2] / 12.0, fu = P.cam.intr[0];
    P.sigma[i] = sqrt(2.0) * sd * sd / (fu * fu);
  }
  if (P.ok) P.ok[i] = ok ? 1 : 0;
}

#endif  // __HIPCC__

// A hypothesis as the kernel keeps it in LDS.  Absolute / relative: h[0..11] the inverse transformation, 3x4 row-major
// (inverseSolution: rotation^T, -(rotation^T) translation; formed once per hypothesis), h[12..14] the translation itself.
// Rotation only: h[0..8] the rotation as it came.
BA_HD void sac_stage_model(int kind, const double* model, double* h) {
  BA_NO_CONTRACT
  if (kind == OKVIS_FE_SAC_ROTATION_ONLY) {
    for (int k = 0; k < 9; ++k) h[k] = model[k];
    return;
  }
  for (int i = 0; i < 3; ++i) {
    const double r0 = model[i], r1 = model[4 + i], r2 = model[8 + i];  // row i of rotation^T
    h[4 * i] = r0, h[4 * i + 1] = r1, h[4 * i + 2] = r2;
    h[4 * i + 3] = ((-r0) * model[3] + (-r1) * model[7]) + (-r2) * model[11];
  }
  h[12] = model[3], h[13] = model[7], h[14] = model[11];
}

BA_HD double sac_dot3(const double* x, const double* y) {
  BA_NO_CONTRACT
  return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

// inverse (3x4) * (p, 1)
BA_HD void sac_apply34(const double* h, const double* p, double* out) {
  BA_NO_CONTRACT
  for (int k = 0; k < 3; ++k) out[k] = ((h[4 * k] * p[0] + h[4 * k + 1] * p[1]) + h[4 * k + 2] * p[2]) + h[4 * k + 3];
}

BA_HD void sac_unit(double* v) {
  BA_NO_CONTRACT
  const double n = sqrt(sac_dot3(v, v));
  v[0] = v[0] / n, v[1] = v[1] / n, v[2] = v[2] / n;
}

BA_HD double sac_sqdist(const double* x, const double* y) {
  BA_NO_CONTRACT
  const double e[3] = {x[0] - y[0], x[1] - y[1], x[2] - y[2]};
  return sac_dot3(e, e);
}

// cam: offset (3), rotation (9); the world point p through the inverse hypothesis into the body, then into its camera
BA_HD double sac_score_absolute(const double* h, const double* p, const double* f, double sigma, const double* cam) {
  BA_NO_CONTRACT
  double body[3];
  sac_apply34(h, p, body);
  const double d[3] = {body[0] - cam[0], body[1] - cam[1], body[2] - cam[2]};
  const double* C = cam + 3;
  double r[3];
  for (int k = 0; k < 3; ++k) r[k] = (C[k] * d[0] + C[3 + k] * d[1]) + C[6 + k] * d[2];  // C^T d
  sac_unit(r);
  return sac_sqdist(r, f) / sigma;
}

BA_HD double sac_score_rotation_only(const double* R, const double* f1, const double* f2, double s1, double s2) {
  BA_NO_CONTRACT
  double f2u[3], f1u[3];
  for (int k = 0; k < 3; ++k) {
    f2u[k] = (R[3 * k] * f2[0] + R[3 * k + 1] * f2[1]) + R[3 * k + 2] * f2[2];
    f1u[k] = (R[k] * f1[0] + R[3 + k] * f1[1]) + R[6 + k] * f1[2];
  }
  return sac_sqdist(f2u, f1) * 0.5 / s1 + sac_sqdist(f1u, f2) * 0.5 / s2;
}

// The two-view midpoint method (not pinned, see the head of this file).  f2' = R12 f2; the points lambda1 f1 and t12 + lambda2 f2'
// closest to each other solve  [f1.f1  -f1.f2'; f1.f2'  -f2'.f2'] (lambda1, lambda2)^T = (t12.f1, t12.f2')^T;  the result is
// their mean.  h holds R12^T in its rotation block: R12(k, j) = h[4 j + k].
BA_HD void sac_midpoint(const double* h, const double* f1, const double* f2, double* p) {
  BA_NO_CONTRACT
  const double* t = h + 12;
  double g[3];
  for (int k = 0; k < 3; ++k) g[k] = (h[k] * f2[0] + h[4 + k] * f2[1]) + h[8 + k] * f2[2];
  const double b0 = sac_dot3(t, f1), b1 = sac_dot3(t, g);
  const double a00 = sac_dot3(f1, f1), a10 = sac_dot3(f1, g), a01 = -a10, a11 = -sac_dot3(g, g);
  const double det = a00 * a11 - a01 * a10;
  const double l0 = (a11 * b0 - a01 * b1) / det, l1 = (a00 * b1 - a10 * b0) / det;
  for (int k = 0; k < 3; ++k) p[k] = (l0 * f1[k] + (t[k] + l1 * g[k])) / 2.0;
}

BA_HD double sac_score_relative(const double* h, const double* f1, const double* f2, double s1, double s2) {
  BA_NO_CONTRACT
  double p[3], r2[3];
  sac_midpoint(h, f1, f2, p);
  sac_apply34(h, p, r2);
  sac_unit(p);
  sac_unit(r2);
  return sac_sqdist(p, f1) * 0.5 / s1 + sac_sqdist(r2, f2) * 0.5 / s2;
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(SAC_THREADS) void sac_consensus_kernel(SacParams P) {
  __shared__ double hyp[SAC_MODEL_TILE * SAC_MODEL_STRIDE];
  const SacJob J = P.jobs[find_job(P.jobs, P.n_jobs, &SacJob::block0)];
  const int local = (int)blockIdx.x - J.block0;
  const int tile = local % J.tiles, m0 = (local / J.tiles) * SAC_MODEL_TILE;
  const int nm = J.n_models - m0 < SAC_MODEL_TILE ? J.n_models - m0 : SAC_MODEL_TILE;
  const int width = J.kind == OKVIS_FE_SAC_ROTATION_ONLY ? 9 : 12;
  if ((int)threadIdx.x < nm) sac_stage_model(J.kind, J.models + (size_t)(m0 + threadIdx.x) * width, hyp + threadIdx.x * SAC_MODEL_STRIDE);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int word = tile * SAC_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (word * 64 >= J.n) return;  // wave-uniform; no barrier follows
  const int i = word * 64 + lane;
  const bool live = i < J.n;
  const size_t n = (size_t)J.n, ii = live ? (size_t)i : n - 1;  // a lane past the end reads the last correspondence and never votes
  const double a[3] = {J.a[ii], J.a[n + ii], J.a[2 * n + ii]};
  const double b[3] = {J.b[ii], J.b[n + ii], J.b[2 * n + ii]};
  const double s1 = J.sigma1[ii];
  double s2 = 0.0, cam[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (J.kind == OKVIS_FE_SAC_ABSOLUTE) {
    const double* c = J.cams + 12 * (size_t)J.cam_index[ii];  // cam_index was checked against n_cams on the host
#pragma unroll
    for (int k = 0; k < 12; ++k) cam[k] = c[k];
  } else {
    s2 = J.sigma2[ii];
  }
  const size_t words = (n + 63) / 64;
  for (int m = 0; m < nm; ++m) {
    const double* h = hyp + m * SAC_MODEL_STRIDE;
    double s;
    if (J.kind == OKVIS_FE_SAC_ABSOLUTE) s = sac_score_absolute(h, a, b, s1, cam);
    else if (J.kind == OKVIS_FE_SAC_ROTATION_ONLY) s = sac_score_rotation_only(h, a, b, s1, s2);
    else s = sac_score_relative(h, a, b, s1, s2);
    const unsigned long long votes = __ballot(live && s < J.threshold);
    if (lane == 0) {
      P.ballots[J.word0 + (int64_t)((size_t)(m0 + m) * words + (size_t)word)] = votes;
      if (votes) atomicAdd(P.counts + J.count0 + m0 + m, __popcll(votes));
    }
    if (J.scores && live) J.scores[(size_t)(m0 + m) * n + (size_t)i] = s;
  }
}

#endif  // __HIPCC__

}  // namespace fe
