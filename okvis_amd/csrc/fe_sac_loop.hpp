// The sampler and the loop of the sample-consensus runs on the device (include/okvis_amd_frontend.h: okvis_fe_ransac): what
// opengv::sac::Ransac<P>::computeModel does around the solvers and the consensus count (okvis_frontend/src/Frontend.cpp:599-611,
// 677-703 are its callers).  OpenGV's source is not part of the reference tree: the sampler and the loop are STATED in the header,
// NOT pinned to OpenGV; this file is that statement in code, and tests/ransac_statement.py is the same statement in numpy.
//
//   sac_sample_kernel   one thread per sample slot, integer arithmetic only: Philox4x32-10 keyed by the job's seed, counter (slot,
//                       block, 0, 0), then a sparse Fisher-Yates over the virtual array A[i] = i whose at most eight touched entries
//                       stay in registers.  Writes the sample table where sac_solve_kernel / sac_gp3p_kernel read it.
//   sac_loop_kernel     one wave per job, no workgroup barrier, no atomics, no scratch memory.  The sequential rule of the header over
//                       the slots in order, in its wave-parallel form: 64 slots per step, a lane per slot; the iteration and skip
//                       counters of a slot are prefix popcounts of the wave's valid ballot, its best-so-far the prefix maximum of the
//                       counts over valid slots (the earlier slot wins a tie), every lane takes the decision of its own slot, and the
//                       first lane that stops ends the walk.  Then the ballot row of the returned hypothesis becomes the ascending
//                       index list (a ballot word per lane, popcounts, a wave prefix sum, scattered writes) and the hypothesis is
//                       copied.  Every loop has a compile-time or argument-bounded count.
//
// The decision functions (sac_philox, sac_draw_sample, sac_done, sac_loop_rule) are BA_HD like the score functions of fe_sac.hpp: a
// plain host compiler sees the same source (tests/ransac_probe.cpp).  sac_done is multiplications, one subtraction and comparisons
// in IEEE double, each rounded on its own (BA_NO_CONTRACT), so that the device, a host compiler and numpy take the same decision.
#pragma once
#include <stdint.h>

#include "../../include/okvis_amd_frontend.h"
#include "ba_math.hpp"
#if defined(__HIPCC__)
#include "fe_kernels.hpp"
#endif

namespace fe {

constexpr int SAC_MAX_SAMPLE = 8;       // the largest sample (relative); two Philox blocks
constexpr int SAC_SAMPLE_THREADS = 64;  // slots per workgroup of sac_sample_kernel
constexpr int SAC_SKIP_FACTOR = 10;     // the loop gives up after 10 * max_iterations invalid samples

BA_HD int sac_sample_size(int kind) {
  return kind == OKVIS_FE_SAC_ABSOLUTE ? OKVIS_FE_SAC_SAMPLE_ABSOLUTE
                                       : kind == OKVIS_FE_SAC_ROTATION_ONLY ? OKVIS_FE_SAC_SAMPLE_ROTATION_ONLY : OKVIS_FE_SAC_SAMPLE_RELATIVE;
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): ten rounds, the key bumped by the Weyl constants between them
BA_HD void sac_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// The sample of slot m of a job with this seed over n correspondences, s of them (s <= 8 and s <= n): distinct indices in
// 0..n-1.  A[k] and A[j] are looked up among the entries touched so far (pos / val; a later entry overrides an earlier one of the
// same position); position k is never visited again, so only A[j] is kept.
BA_HD void sac_draw_sample(uint64_t seed, uint32_t m, uint32_t n, int s, int32_t* sample) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t u[SAC_MAX_SAMPLE] = {0, 0, 0, 0, 0, 0, 0, 0};
  sac_philox(m, 0u, 0u, 0u, k0, k1, u);
  if (s > 4) sac_philox(m, 1u, 0u, 0u, k0, k1, u + 4);
  uint32_t pos[SAC_MAX_SAMPLE], val[SAC_MAX_SAMPLE];
#pragma unroll
  for (int k = 0; k < SAC_MAX_SAMPLE; ++k) {
    if (k >= s) break;
    const uint32_t j = (uint32_t)k + (uint32_t)(((uint64_t)u[k] * (uint64_t)(n - (uint32_t)k)) >> 32);
    uint32_t aj = j, ak = (uint32_t)k;
#pragma unroll
    for (int t = 0; t < SAC_MAX_SAMPLE; ++t) {
      if (t >= k) break;
      if (pos[t] == j) aj = val[t];
      if (pos[t] == (uint32_t)k) ak = val[t];
    }
    pos[k] = j, val[k] = ak;
    sample[k] = (int32_t)aj;
  }
}

// The adaptive bound it >= log(1 - p) / log(1 - w^s), w = c / n, without transcendental functions: (1 - w^s)^it <= 1 - p.
// c = 0 never satisfies it (q clamps to 1 - 2^-52, whose powers stay above 1 - p for every it the loop reaches).
BA_HD bool sac_done(int it, int c, int n, int s, double p) {
  BA_NO_CONTRACT
  const double w = (double)c / (double)n;
  double ws = w;
  for (int k = 1; k < s; ++k) ws = ws * w;
  double q = 1.0 - ws;
  const double lo = 2.220446049250313e-16, hi = 1.0 - 2.220446049250313e-16;  // 2^-52, 1 - 2^-52
  q = q < lo ? lo : (q > hi ? hi : q);
  double r = 1.0, b = q;
  for (uint32_t e = (uint32_t)it; e; e >>= 1) {
    if (e & 1u) r = r * b;
    b = b * b;
  }
  return r <= 1.0 - p;
}

struct SacLoopState {  // the loop's variables
  int32_t best, best_count, iterations, skipped, stop;
};

// The sequential rule of the header, slot by slot.
BA_HD SacLoopState sac_loop_rule(const int32_t* counts, const uint8_t* valid, int n_slots, int n, int s, int max_iterations, double p) {
  SacLoopState L = {-1, -1, 0, 0, OKVIS_FE_RANSAC_STOP_EXHAUSTED};
  for (int m = 0; m < n_slots; ++m) {
    if (!valid[m]) {
      L.skipped += 1;
      if ((int64_t)L.skipped >= (int64_t)SAC_SKIP_FACTOR * max_iterations) {
        L.stop = OKVIS_FE_RANSAC_STOP_SKIPS;
        break;
      }
      continue;
    }
    if (counts[m] > L.best_count) L.best = m, L.best_count = counts[m];
    L.iterations += 1;
    if (sac_done(L.iterations, L.best_count, n, s, p)) {
      L.stop = OKVIS_FE_RANSAC_STOP_CONVERGED;
      break;
    }
    if (L.iterations > max_iterations) {
      L.stop = OKVIS_FE_RANSAC_STOP_MAX_ITERATIONS;
      break;
    }
  }
  return L;
}

#if defined(__HIPCC__)
struct SampleJob {  // one job of sac_sample_kernel, device pointers
  int32_t* samples;  // [n_slots][s]
  uint64_t seed;
  int32_t n, n_slots, s;
  int32_t block0;    // first workgroup of the job in the grid
};

struct SampleParams {
  const SampleJob* jobs;
  int32_t n_jobs;
};

struct LoopRecord {  // what a job hands back besides its inlier list
  int32_t best, n_inliers, iterations, skipped, stop, reserved;
  double model[12];
};

struct LoopJob {  // one job of sac_loop_kernel, device pointers
  const int32_t* counts;               // [n_slots], as sac_consensus_kernel left them
  const uint8_t* valid;                // [n_slots], as the solver kernel left them
  const unsigned long long* ballots;   // [n_slots][ceil(n / 64)]
  const double* models;                // [n_slots][width]
  int32_t* inliers;                    // [n] or null
  LoopRecord* record;
  double probability;
  int32_t n, n_slots, s, max_iterations, width;
};

struct LoopParams {
  const LoopJob* jobs;
  int32_t n_jobs;
};

__global__ __launch_bounds__(SAC_SAMPLE_THREADS) void sac_sample_kernel(SampleParams P) {
  const SampleJob J = P.jobs[find_job(P.jobs, P.n_jobs, &SampleJob::block0)];
  const int m = ((int)blockIdx.x - J.block0) * SAC_SAMPLE_THREADS + (int)threadIdx.x;
  if (m >= J.n_slots) return;
  int32_t q[SAC_MAX_SAMPLE];
  sac_draw_sample(J.seed, (uint32_t)m, (uint32_t)J.n, J.s, q);
  int32_t* dst = J.samples + (size_t)m * (size_t)J.s;
#pragma unroll
  for (int k = 0; k < SAC_MAX_SAMPLE; ++k)
    if (k < J.s) dst[k] = q[k];
}

// One wave per workgroup, one workgroup per job.
__global__ __launch_bounds__(64) void sac_loop_kernel(LoopParams P) {
  if ((int)blockIdx.x >= P.n_jobs) return;
  const LoopJob J = P.jobs[blockIdx.x];
  const int lane = threadIdx.x;
  const unsigned long long upto = ~0ull >> (63 - lane);  // lanes 0..lane
  const int64_t skip_limit = (int64_t)SAC_SKIP_FACTOR * J.max_iterations;
  SacLoopState L = {-1, -1, 0, 0, OKVIS_FE_RANSAC_STOP_EXHAUSTED};
  for (int m0 = 0; m0 < J.n_slots; m0 += 64) {  // at most 16 steps
    const int m = m0 + lane;
    const bool live = m < J.n_slots;
    const bool ok = live && J.valid[m] != 0;
    const unsigned long long oks = __ballot(ok), bad = __ballot(live && !ok);
    const int it = L.iterations + __popcll(oks & upto), skipped = L.skipped + __popcll(bad & upto);
    // the best hypothesis among the valid slots up to this lane: an inclusive prefix maximum, the earlier slot on a tie
    int bc = ok ? J.counts[m] : -1, bi = ok ? m : -1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int oc = __shfl_up(bc, d), oi = __shfl_up(bi, d);
      if (lane >= d && oc >= bc && oi >= 0) bc = oc, bi = oi;  // oc == bc: the lower lanes hold the earlier slot
    }
    if (bc <= L.best_count) bc = L.best_count, bi = L.best;  // the carried best is earlier still
    int stop = -1;
    if (live) {
      if (!ok) {
        if ((int64_t)skipped >= skip_limit) stop = OKVIS_FE_RANSAC_STOP_SKIPS;
      } else if (sac_done(it, bc, J.n, J.s, J.probability)) {
        stop = OKVIS_FE_RANSAC_STOP_CONVERGED;
      } else if (it > J.max_iterations) {
        stop = OKVIS_FE_RANSAC_STOP_MAX_ITERATIONS;
      }
    }
    const unsigned long long stops = __ballot(stop >= 0);
    const int last = J.n_slots - m0 < 64 ? J.n_slots - m0 - 1 : 63;
    const int from = stops ? __builtin_ctzll(stops) : last;  // wave-uniform
    L.best = __shfl(bi, from), L.best_count = __shfl(bc, from), L.iterations = __shfl(it, from), L.skipped = __shfl(skipped, from);
    if (stops) {
      L.stop = __shfl(stop, from);
      break;
    }
  }
  const int n_inliers = L.best >= 0 ? L.best_count : 0;
  LoopRecord* R = J.record;
  if (lane == 0) {
    R->best = L.best, R->n_inliers = n_inliers, R->iterations = L.iterations, R->skipped = L.skipped, R->stop = L.stop;
    R->reserved = 0;
  }
  if (lane < 12) R->model[lane] = (L.best >= 0 && lane < J.width) ? J.models[(size_t)L.best * (size_t)J.width + lane] : __builtin_nan("");
  if (!J.inliers || L.best < 0) return;
  // row `best` of the ballots into ascending indices: a word per lane, 64 words per step
  const int words = (J.n + 63) / 64;
  const unsigned long long* row = J.ballots + (size_t)L.best * (size_t)words;
  int base = 0;
  for (int w0 = 0; w0 < words; w0 += 64) {  // at most 16 steps
    const int w = w0 + lane;
    unsigned long long votes = w < words ? row[w] : 0ull;
    const int mine = __popcll(votes);
    int before = mine;  // inclusive prefix sum
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(before, d);
      if (lane >= d) before += o;
    }
    const int total = __shfl(before, 63);
    int at = base + before - mine;
    for (int b = 0; b < 64 && votes; ++b, votes &= votes - 1) J.inliers[at++] = w * 64 + __builtin_ctzll(votes);
    base += total;
  }
}
#endif  // __HIPCC__

}  // namespace fe
