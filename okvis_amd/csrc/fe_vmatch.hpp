// Verified matching on the device (include/okvis_amd_frontend.h: okvis_fe_match_verified): the dense matcher's per-row lists under the
// distance VioKeyframeWindowMatchingAlgorithm<G>::distance defines — the Hamming distance where it is under the threshold AND
// verifyMatch(a, b) holds, FLT_MAX elsewhere (okvis_frontend/include/okvis/VioKeyframeWindowMatchingAlgorithm.hpp, distance;
// okvis_frontend/src/VioKeyframeWindowMatchingAlgorithm.cpp:307-337).
//
//   vmatch_prepass_kernel        everything that depends on one keypoint only, for all jobs of a call.
//                                2D-2D: the normalised ray of every keypoint of A and the normalised C_AB ray of every keypoint of B
//                                (the first lines of stereoTriangulate, ProbabilisticStereoTriangulator.cpp:191-205).
//                                3D-2D: uv, U and the projection status of every row of A in play (doSetup :165-213:
//                                project_landmark, as project_landmarks_kernel).
//   verified_lists_kernel<W>     layout of best_lists_kernel: one wave per row of A, B staged through LDS in tiles of 256, the list
//                                wave-uniform in registers.  A pair has to be verified only if it is in play, d < threshold and
//                                d < the list's last entry at the start of the tile (the last entry only falls).  Those few pairs of
//                                the whole tile are gathered into consecutive slots of a per-wave queue in LDS, verified with all
//                                lanes busy, and the survivors inserted in slot order = ascending b, each one checked again against the
//                                last entry it finds: the sequence of the reference.  The fp64 geometry never runs under the sparse
//                                mask of the distance loop.
// The geometry is not restated here: project_landmark, verify_2d2d and gate_3d2d (fe_kernels.hpp) are the functions
// project_landmarks_kernel, stereo_triangulate_kernel and gate_3d2d_kernel call, so a decision here is the decision the stand-alone
// entries take for that pair.  One exception, five lines: the product U = J P3 J^T behind project_landmark is written out in both
// kernels (fe_kernels.hpp says why).  No atomics; nothing depends on scheduling.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "fe_kernels.hpp"
#include "fe_match.hpp"

namespace fe {

constexpr int VMATCH_PRE_THREADS = 256;

struct VJob {  // one matching step of okvis_fe_match_verified, device pointers
  const uint8_t* desc_a;
  const uint8_t* desc_b;
  const uint8_t* skip_a;
  const uint8_t* skip_b;
  const float* kp_a;  // [n_a][3]; nullptr where a 3D-2D step came without
  const float* kp_b;
  const double* hp_W;   // 3D-2D [n_a][4]
  const double* sig_a;  // 2D-2D [n_a] raySigmasA_
  const double* sig_b;  // 2D-2D [n_b] raySigmasB_
  double* ray_a;        // 2D-2D [n_a][3]
  double* ray_b;        // 2D-2D [n_b][3], already in frame A
  double* uv;           // 3D-2D [n_a][2]
  double* U;            // 3D-2D [n_a][4]
  uint8_t* status;      // 3D-2D [n_a]
  Camera cam_a, cam_b;
  double T[7];  // T_AB (2D-2D) or T_CbW (3D-2D)
  double P3[9];
  int32_t kind, n_a, n_b;
  int32_t block0;  // first workgroup of the job in the grid of verified_lists_kernel
  int32_t row0;    // first row of the job in the lists
  int32_t pre0;    // first workgroup of the job in the grid of vmatch_prepass_kernel
};

struct VListParams {
  const VJob* jobs;
  int32_t n_jobs;
  float threshold, initial;  // as BestParams
  int32_t num_best;
  int32_t* list_idx;  // [rows][num_best]
  float* list_dist;
  double* list_chi2;    // 3D-2D: the chi2 of the entry's gate
  uint8_t* list_flags;  // 3D-2D: its OKVIS_FE_GATE_* bits
};

__global__ __launch_bounds__(VMATCH_PRE_THREADS) void vmatch_prepass_kernel(const VJob* jobs, int n_jobs) {
  const VJob& J = jobs[find_job(jobs, n_jobs, &VJob::pre0)];
  const int i = ((int)blockIdx.x - J.pre0) * VMATCH_PRE_THREADS + (int)threadIdx.x;
  if (J.kind == OKVIS_FE_MATCH_2D2D) {
    if (i < J.n_a) {
      const float* ka = J.kp_a + 3 * i;
      double dA[3];
      back_project(J.cam_a, (double)ka[0], (double)ka[1], dA);
      normalize3(dA);
      J.ray_a[3 * i] = dA[0], J.ray_a[3 * i + 1] = dA[1], J.ray_a[3 * i + 2] = dA[2];
    } else if (i < J.n_a + J.n_b) {
      const int b = i - J.n_a;
      const float* kb = J.kp_b + 3 * b;
      double dB[3], C_AB[9], dBA[3];
      back_project(J.cam_b, (double)kb[0], (double)kb[1], dB);
      qrot(J.T + 3, C_AB);
      mat3_vec(C_AB, dB, dBA);
      normalize3(dBA);
      J.ray_b[3 * b] = dBA[0], J.ray_b[3 * b + 1] = dBA[1], J.ray_b[3 * b + 2] = dBA[2];
    }
    return;
  }
  // doSetup, Match3D2D (:177-205): the projection for the rows in play, zeros for the others
  if (i >= J.n_a) return;
  double uv[2] = {0, 0}, U[4] = {0, 0, 0, 0};
  int st = 0;
  if (!(J.skip_a && J.skip_a[i])) {
    double Jc[6] = {0, 0, 0, 0, 0, 0}, JP[6];
    st = project_landmark(J.cam_b, J.T, J.hp_W + 4 * i, uv, Jc);
    for (int r = 0; r < 2; ++r)  // U = J P3 J^T, as project_landmarks_kernel writes it out
      for (int c = 0; c < 3; ++c) JP[3 * r + c] = Jc[3 * r] * J.P3[c] + Jc[3 * r + 1] * J.P3[3 + c] + Jc[3 * r + 2] * J.P3[6 + c];
    for (int r = 0; r < 2; ++r)
      for (int c = 0; c < 2; ++c) U[2 * r + c] = JP[3 * r] * Jc[3 * c] + JP[3 * r + 1] * Jc[3 * c + 1] + JP[3 * r + 2] * Jc[3 * c + 2];
  }
  J.status[i] = (uint8_t)st;
  J.uv[2 * i] = uv[0], J.uv[2 * i + 1] = uv[1];
  for (int k = 0; k < 4; ++k) J.U[4 * i + k] = U[k];
}

template <int W>
__global__ __launch_bounds__(MATCH_THREADS) void verified_lists_kernel(VListParams P) {
  __shared__ uint4 lds[W * MATCH_TILE];
  __shared__ uint32_t queue[MATCH_WAVES][MATCH_TILE];  // per row: (index in the tile << 16) | distance of the pairs to verify
  const VJob& J = P.jobs[find_job(P.jobs, P.n_jobs, &VJob::block0)];
  const int n_a = J.n_a, n_b = J.n_b;
  const bool is2d = J.kind == OKVIS_FE_MATCH_2D2D;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = ((int)blockIdx.x - J.block0) * MATCH_WAVES + wave;
  bool live = row < n_a && !(J.skip_a && J.skip_a[row]);
  if (live && !is2d) live = J.status[row] == OKVIS_FE_PROJ_SUCCESSFUL;
  const int nb = P.num_best;
  uint4 a[W] = {};
  // what the verification reads of the row
  double ra[3] = {0, 0, 0}, sig_a = 0, C_AB[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, uv[2] = {0, 0}, U[4] = {0, 0, 0, 0};
  float ka[3] = {0, 0, 0};
  if (live) {
    load_row<W>(a, J.desc_a, row);
    if (is2d) {
      for (int k = 0; k < 3; ++k) ra[k] = J.ray_a[3 * row + k], ka[k] = J.kp_a[3 * row + k];
      sig_a = J.sig_a[row];
      qrot(J.T + 3, C_AB);
    } else {
      uv[0] = J.uv[2 * row], uv[1] = J.uv[2 * row + 1];
      for (int k = 0; k < 4; ++k) U[k] = J.U[4 * row + k];
    }
  }
  float ld[MATCH_MAX_BEST];
  int li[MATCH_MAX_BEST];
  double lc[MATCH_MAX_BEST];
  unsigned lf[MATCH_MAX_BEST];
#pragma unroll
  for (int j = 0; j < MATCH_MAX_BEST; ++j) ld[j] = P.initial, li[j] = -1, lc[j] = 0.0, lf[j] = 0u;
  float last = P.initial;
  uint32_t* q = queue[wave];
  for (int b0 = 0; b0 < n_b; b0 += MATCH_TILE) {
    stage_tile<W>(lds, J.desc_b, b0, n_b);
    __syncthreads();
    if (live) {
      int total = 0;  // pairs of this row and tile that have to be verified; their slots are in ascending b
#pragma unroll
      for (int s = 0; s < MATCH_TILE / 64; ++s) {
        const int t = s * 64 + lane, b = b0 + t;
        if (b0 + s * 64 >= n_b) break;
        const bool in = b < n_b && !(J.skip_b && J.skip_b[b]);
        const int d = hamming_lds<W>(a, lds, t);
        const bool cand = in && (float)d < P.threshold && (float)d < last;
        const unsigned long long m = __ballot(cand);
        if (cand) q[total + __popcll(m & ((1ull << lane) - 1ull))] = ((uint32_t)t << 16) | (uint32_t)d;
        total += __popcll(m);
      }
      // the queue is written and read by this wave only: order the two within the wave
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int base = 0; base < total; base += 64) {
        const bool have = base + lane < total;
        const uint32_t e = have ? q[base + lane] : 0u;
        const int b = b0 + (int)(e >> 16);
        const float fd = (float)(e & 0xffffu);
        bool ok = false;
        double chi2 = 0.0;
        unsigned fl = 0u;
        if (have) {
          const float* kb = J.kp_b + 3 * b;
          if (is2d) {
            const double rb[3] = {J.ray_b[3 * b], J.ray_b[3 * b + 1], J.ray_b[3 * b + 2]};
            const double sig_b = J.sig_b[b];
            double hp[4];
            bool parallel, hp_assigned;
            ok = verify_2d2d(J.cam_a, J.cam_b, J.T, C_AB, ka, kb, ra, rb, sig_a > sig_b ? sig_a : sig_b, hp, &parallel, &hp_assigned);
          } else {
            fl = gate_3d2d(uv, U, kb, &chi2);
            ok = (fl & OKVIS_FE_GATE_VERIFIED) != 0u;
          }
        }
        unsigned long long m = __ballot(ok);
        while (m) {
          const int l = __ffsll((long long)m) - 1;
          m &= m - 1;
          const float dv = __shfl(fd, l);
          if (!(dv < last)) continue;
          const int bv = __shfl(b, l);
          const double cv = __shfl(chi2, l);
          const unsigned fv = __shfl(fl, l);
          int pos = 0;  // std::lower_bound: the entries of strictly smaller distance stay in front
#pragma unroll
          for (int j = 0; j < MATCH_MAX_BEST; ++j) pos += (j < nb && ld[j] < dv) ? 1 : 0;
#pragma unroll
          for (int j = MATCH_MAX_BEST - 1; j >= 1; --j)
            if (j < nb) {
              if (j > pos) ld[j] = ld[j - 1], li[j] = li[j - 1], lc[j] = lc[j - 1], lf[j] = lf[j - 1];
              else if (j == pos) ld[j] = dv, li[j] = bv, lc[j] = cv, lf[j] = fv;
            }
          if (pos == 0) ld[0] = dv, li[0] = bv, lc[0] = cv, lf[0] = fv;
#pragma unroll
          for (int j = 0; j < MATCH_MAX_BEST; ++j)
            if (j == nb - 1) last = ld[j];
        }
      }
    }
    __syncthreads();
  }
  if (row < n_a && lane == 0) {
    const size_t o = (size_t)(J.row0 + row) * (size_t)nb;
#pragma unroll
    for (int j = 0; j < MATCH_MAX_BEST; ++j)
      if (j < nb) {
        P.list_idx[o + j] = li[j], P.list_dist[o + j] = ld[j];
        P.list_chi2[o + j] = lc[j], P.list_flags[o + j] = (uint8_t)lf[j];
      }
  }
}

}  // namespace fe
