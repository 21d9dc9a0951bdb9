// Descriptor matching on the device (include/okvis_amd_frontend.h: okvis_fe_hamming_candidates, okvis_fe_match_descriptors).
//
// Binary descriptors of W x 16 bytes (W = 1..4; BRISK is 3), distance = popcount of the XOR (brisk::Hamming::PopcntofXORed).
// One wave per keypoint of image A: its descriptor is wave-uniform, the 64 lanes take 64 consecutive keypoints of image B.  The
// MATCH_WAVES rows of a workgroup share a tile of B staged in LDS, stored word-major (lds[w][b]) so that the 64 lanes of a wave
// read 64 consecutive uint4.  Everything is integer and in a fixed order: no atomics, the order of the output does not depend on
// scheduling.
//   hamming_rows_kernel<W, false>   per row, the number of pairs under the threshold
//   row_offsets_kernel              exclusive scan of those counts (one workgroup; at most 65536 rows)
//   hamming_rows_kernel<W, true>    the distances again (cheaper than storing the matrix), each kept pair to its slot: row offset +
//                                   pairs kept in earlier 64-blocks of the row + prefix popcount of the ballot = ascending (a, b)
//   best_lists_kernel<W>            for all (job, row tile) of a call: the list DenseMatcher::listBIteration leaves after scanning b
//                                   in ascending order (okvis_matcher/include/okvis/implementation/DenseMatcher.hpp:153-179)
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "fe_kernels.hpp"

namespace fe {

constexpr int MATCH_WAVES = 4;                   // rows of A per workgroup, one wave each
constexpr int MATCH_THREADS = 64 * MATCH_WAVES;
constexpr int MATCH_TILE = 256;                  // descriptors of B in LDS at a time (W * 4 KiB)
constexpr int MATCH_MAX_BEST = 8;
constexpr int SCAN_THREADS = 1024;

struct CandParams {
  const uint8_t* desc_a;
  const uint8_t* desc_b;
  const uint8_t* skip_a;  // nullptr = none
  const uint8_t* skip_b;
  int32_t n_a, n_b;
  float threshold;
  int32_t* counts;                    // [n_a]
  const unsigned long long* offsets;  // [n_a] exclusive scan of counts
  long long capacity;
  int32_t* pairs;  // [capacity][2]
  float* dist;     // [capacity]
};

struct MatchJob {  // one (image A, image B) of okvis_fe_match_descriptors, device pointers
  const uint8_t* desc_a;
  const uint8_t* desc_b;
  const uint8_t* skip_a;
  const uint8_t* skip_b;
  int32_t n_a, n_b;
  int32_t block0;  // first workgroup of the job in the grid
  int32_t row0;    // first row of the job in list_idx / list_dist
};

struct BestParams {
  const MatchJob* jobs;
  int32_t n_jobs;
  float threshold;  // distance(a, b) = Hamming distance where it is < threshold, FLT_MAX elsewhere
  float initial;    // distance of the (-1, .) entries a list starts with: threshold, or FLT_MAX under the ratio rule
  int32_t num_best;
  int32_t* list_idx;  // [rows][num_best]
  float* list_dist;
};

// tile [b0, b0 + MATCH_TILE) of B into LDS, coalesced from global, word-major in LDS
template <int W>
__device__ inline void stage_tile(uint4* lds, const uint8_t* desc_b, int b0, int n_b) {
  const uint4* g = reinterpret_cast<const uint4*>(desc_b) + (size_t)b0 * W;
  const int n = (n_b - b0 < MATCH_TILE ? n_b - b0 : MATCH_TILE) * W;
  for (int f = threadIdx.x; f < n; f += MATCH_THREADS) {
    const int b = f / W, w = f - b * W;
    lds[w * MATCH_TILE + b] = g[f];
  }
}

template <int W>
__device__ inline int hamming_lds(const uint4 (&a)[W], const uint4* lds, int t) {
  int d = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const uint4 x = lds[w * MATCH_TILE + t];
    d += __popcll(((unsigned long long)(x.y ^ a[w].y) << 32) | (unsigned long long)(x.x ^ a[w].x));
    d += __popcll(((unsigned long long)(x.w ^ a[w].w) << 32) | (unsigned long long)(x.z ^ a[w].z));
  }
  return d;
}

template <int W>
__device__ inline void load_row(uint4 (&a)[W], const uint8_t* desc_a, int row) {
  const uint4* g = reinterpret_cast<const uint4*>(desc_a) + (size_t)row * W;
#pragma unroll
  for (int w = 0; w < W; ++w) a[w] = g[w];
}

template <int W, bool WRITE>
__global__ __launch_bounds__(MATCH_THREADS) void hamming_rows_kernel(CandParams P) {
  __shared__ uint4 lds[W * MATCH_TILE];
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * MATCH_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool live = row < P.n_a && !(P.skip_a && P.skip_a[row]);
  uint4 a[W] = {};
  if (live) load_row<W>(a, P.desc_a, row);
  const unsigned long long base = (WRITE && live) ? P.offsets[row] : 0ull;
  int kept = 0;  // pairs of this row in the 64-blocks before the current one
  for (int b0 = 0; b0 < P.n_b; b0 += MATCH_TILE) {
    stage_tile<W>(lds, P.desc_b, b0, P.n_b);
    __syncthreads();
    if (live) {
#pragma unroll
      for (int s = 0; s < MATCH_TILE / 64; ++s) {
        const int t = s * 64 + lane, b = b0 + t;
        if (b0 + s * 64 >= P.n_b) break;
        const bool in = b < P.n_b && !(P.skip_b && P.skip_b[b]);
        const int d = hamming_lds<W>(a, lds, t);
        const bool keep = in && (float)d < P.threshold;
        const unsigned long long m = __ballot(keep);
        if (WRITE && keep) {
          const unsigned long long slot = base + (unsigned long long)(kept + __popcll(m & ((1ull << lane) - 1ull)));
          if (slot < (unsigned long long)P.capacity) {
            P.pairs[2 * slot] = row, P.pairs[2 * slot + 1] = b;
            if (P.dist) P.dist[slot] = (float)d;
          }
        }
        kept += __popcll(m);
      }
    }
    __syncthreads();
  }
  if (!WRITE && row < P.n_a && lane == 0) P.counts[row] = kept;
}

// offsets[i] = sum of counts[0..i), *total = the sum of all; one workgroup of SCAN_THREADS
__global__ __launch_bounds__(SCAN_THREADS) void row_offsets_kernel(const int32_t* counts, unsigned long long* offsets,
                                                                    unsigned long long* total, int n) {
  __shared__ unsigned long long part[SCAN_THREADS];
  const int t = threadIdx.x, per = (n + SCAN_THREADS - 1) / SCAN_THREADS;
  const int lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
  unsigned long long s = 0;
  for (int i = lo; i < hi; ++i) s += (unsigned long long)counts[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < SCAN_THREADS; off <<= 1) {
    const unsigned long long v = t >= off ? part[t - off] : 0ull;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned long long run = part[t] - s;
  for (int i = lo; i < hi; ++i) {
    offsets[i] = run;
    run += (unsigned long long)counts[i];
  }
  if (t == SCAN_THREADS - 1) *total = part[t];
}

// The list is kept by every lane of the row's wave in registers (all values are wave-uniform).  A 64-block of B is reduced to the
// ballot of the lanes that beat the list's last entry; those few are inserted one by one in ascending b, each one checked again
// against the last entry it left behind: exactly the sequence of the reference, ties included (a candidate equal to the last
// entry is turned away, one that goes in is placed in front of entries of its own distance).
template <int W>
__global__ __launch_bounds__(MATCH_THREADS) void best_lists_kernel(BestParams P) {
  __shared__ uint4 lds[W * MATCH_TILE];
  const MatchJob J = P.jobs[find_job(P.jobs, P.n_jobs, &MatchJob::block0)];
  const int lane = threadIdx.x & 63;
  const int row = ((int)blockIdx.x - J.block0) * MATCH_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool live = row < J.n_a && !(J.skip_a && J.skip_a[row]);
  const int nb = P.num_best;
  uint4 a[W] = {};
  if (live) load_row<W>(a, J.desc_a, row);
  float ld[MATCH_MAX_BEST];
  int li[MATCH_MAX_BEST];
#pragma unroll
  for (int j = 0; j < MATCH_MAX_BEST; ++j) ld[j] = P.initial, li[j] = -1;
  float last = P.initial;
  for (int b0 = 0; b0 < J.n_b; b0 += MATCH_TILE) {
    stage_tile<W>(lds, J.desc_b, b0, J.n_b);
    __syncthreads();
    if (live) {
#pragma unroll
      for (int s = 0; s < MATCH_TILE / 64; ++s) {
        const int t = s * 64 + lane, b = b0 + t;
        if (b0 + s * 64 >= J.n_b) break;
        const bool in = b < J.n_b && !(J.skip_b && J.skip_b[b]);
        const float d = (float)hamming_lds<W>(a, lds, t);
        const float fd = (in && d < P.threshold) ? d : FLT_MAX;
        unsigned long long m = __ballot(fd < last);
        while (m) {
          const int l = __ffsll((long long)m) - 1;
          m &= m - 1;
          const float dv = __shfl(fd, l);
          if (!(dv < last)) continue;
          const int bv = b0 + s * 64 + l;
          int pos = 0;  // std::lower_bound: the entries of strictly smaller distance stay in front
#pragma unroll
          for (int j = 0; j < MATCH_MAX_BEST; ++j) pos += (j < nb && ld[j] < dv) ? 1 : 0;
#pragma unroll
          for (int j = MATCH_MAX_BEST - 1; j >= 1; --j)
            if (j < nb) {
              if (j > pos) ld[j] = ld[j - 1], li[j] = li[j - 1];
              else if (j == pos) ld[j] = dv, li[j] = bv;
            }
          if (pos == 0) ld[0] = dv, li[0] = bv;
#pragma unroll
          for (int j = 0; j < MATCH_MAX_BEST; ++j)
            if (j == nb - 1) last = ld[j];
        }
      }
    }
    __syncthreads();
  }
  if (row < J.n_a && lane == 0) {
    const size_t o = (size_t)(J.row0 + row) * (size_t)nb;
#pragma unroll
    for (int j = 0; j < MATCH_MAX_BEST; ++j)
      if (j < nb) P.list_idx[o + j] = li[j], P.list_dist[o + j] = ld[j];
  }
}

}  // namespace fe
