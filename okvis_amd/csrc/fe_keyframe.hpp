// The keyframe decision of the OKVIS frontend on the device (include/okvis_amd_frontend.h: okvis_fe_keyframe_decision): what
// Frontend::doWeNeedANewKeyframe (okvis_frontend/src/Frontend.cpp:295-369) computes per camera image — the convex hull of all
// keypoints and of the keypoints that carry a landmark, the two hull areas, the number of keypoints strictly inside the matched
// hull — for the images of many multiframes in one launch.  The fold over a multiframe's images (:359-360) and the comparison
// with the thresholds (:364-368) are a few operations per job and run on the host from the per-image records (kf_fold).
//
// cv::convexHull, cv::contourArea and cv::pointPolygonTest are OpenCV's, and OpenCV's source is not part of the reference tree:
// the three are stated from their mathematical definitions (the header says how) and are NOT pinned to OpenCV.  Keypoints are
// float, so every quantity below has an exact rational value, and the statement is exact: the hull and the inside count do not
// depend on rounding, the areas are one fixed sequence of IEEE double operations.
//
//   kf_orient_sign  the exact sign of (bx-ax)(cy-ay) - (by-ay)(cx-ax): a double filter with a proven bound, then an exact expansion
//   kf_pick         the comparator of the gift wrapping around a hull vertex c: "more clockwise, or collinear and farther", ties
//                   (equal coordinates) to the lower index.  A strict weak order on the points that differ from c, because c is an
//                   extreme point and all others lie within an angle below 180 degrees: any reduction tree gives the same winner.
//   kf_shoelace     the area sum in hull order, every product exact, every sum rounded once, no fused multiply-add
//   kf_image_serial the whole per-image statement as a plain loop (host referee of the probe and CPU side of the benchmark)
//
// keyframe_kernel: ONE WAVE PER IMAGE, one wave per workgroup, no workgroup barrier, no atomics, no scratch.  The coordinates sit
// in the wave's LDS (8 bytes per keypoint, 64 KB at the limit of 8192).  Per hull vertex every lane scans its share of the points
// under kf_pick, a 6-step butterfly reduces the 64 candidates (every lane ends with the same winner).  The hull's index list goes
// to global memory: EVERY lane stores the (wave-uniform) index to the same address, so every lane later reads only what it has
// written itself, and no fence is needed for it.  The scans read LDS and registers only (a lane's matched flags are two mask words);
// the shoelace sum and the inside test read the list back 64 vertices at a time and pass them round by shuffle.
// Work: O(n h) predicates per hull and for the inside test, at most 8192^2 each (profiles/keyframe_notes.md).
//
// The predicates are BA_HD like ba_math.hpp's: a plain host compiler sees them too; the kernel is for hipcc only.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ba_math.hpp"

#if defined(__HIPCC__)
#define KF_NOINLINE __host__ __device__ __attribute__((noinline))
#else
#define KF_NOINLINE __attribute__((noinline))
#endif

namespace fe {

constexpr int KF_MAX_KEYPOINTS = 8192;  // per image
constexpr int KF_MAX_CAMS = 8;          // per job
constexpr int KF_FEW_POINTS = 1, KF_FEW_MATCHES = 2;  // OKVIS_FE_KF_*

struct KfPoint { float x, y; };

// s = a + b exactly: s + e with s = fl(a + b) (Knuth's two-sum; exact for all doubles unless the sum overflows)
BA_HD void kf_two_sum(double a, double b, double* s, double* e) {
  BA_NO_CONTRACT
  const double x = a + b;
  const double bv = x - a;
  const double av = x - bv;
  *s = x;
  *e = (a - av) + (b - bv);
}

// The exact path.  det = (bx cy - by cx) + (ay cx - ax cy) + (ax by - ay bx): six products of two floats, each exact in double (48
// significant bits; magnitudes within 2^-298 .. 2^256, far from double's limits).  They are summed into a non-overlapping expansion
// (Shewchuk's Grow-Expansion: each new term runs through the components with two-sum, smallest first); partial sums stay below
// 6 * 2^256, so two-sum never overflows and the expansion's value is the exact sum.  Its components do not overlap and ascend in
// magnitude, so the sign of the sum is the sign of the last non-zero one.  Holds for every finite float.  Rare: kept out of line.
KF_NOINLINE inline int kf_orient_exact(double ax, double ay, double bx, double by, double cx, double cy) {
  BA_NO_CONTRACT
  const double t[6] = {bx * cy, -(by * cx), ay * cx, -(ax * cy), ax * by, -(ay * bx)};
  double e[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double q = t[k];
#pragma unroll
    for (int i = 0; i < k; ++i) kf_two_sum(q, e[i], &q, &e[i]);
    e[k] = q;
  }
#pragma unroll
  for (int i = 5; i >= 0; --i)
    if (e[i] != 0.0) return e[i] > 0.0 ? 1 : -1;
  return 0;
}

// orient(a, b, c): +1 where c lies to the left of a -> b, -1 to the right, 0 on the line; exact over the rationals the floats are.
// The fast path, with u = 2^-53: the four differences of floats are computed in double with relative error <= u each (no
// underflow: a difference of floats is a multiple of 2^-149; no overflow: below 2^129), the products l, r with one more (products
// are 0 or within 2^-298 .. 2^258: no underflow, no overflow), so |l - L| <= ((1+u)^3 - 1) |L| and |L| <= |l| / (1-u)^3, and the same
// for r; det = fl(l - r) adds u |l - r|.  Together |det - (L - R)| <= (3u + 16u^2) (|l| + |r|) — the bound of Shewchuk's orient2d
// ("Adaptive Precision Floating-Point Arithmetic and Fast Robust Geometric Predicates", 1997, ccwerrboundA), which covers doubles
// and therefore floats.  Where |det| exceeds it the sign of det is the exact sign; elsewhere (det = 0 included) the exact path.
BA_HD int kf_orient_sign(KfPoint a, KfPoint b, KfPoint c) {
  BA_NO_CONTRACT
  const double ax = a.x, ay = a.y, bx = b.x, by = b.y, cx = c.x, cy = c.y;
  const double l = (bx - ax) * (cy - ay), r = (by - ay) * (cx - ax);
  const double det = l - r;
  const double bound = 3.3306690738754716e-16 * (fabs(l) + fabs(r));  // (3 + 16u) u, rounded up
  if (det > bound) return 1;
  if (-det > bound) return -1;
  // two of the three coincide: 0 without the expansion.  Common, not rare: the butterfly of the gift wrapping compares a candidate
  // with itself once it has spread over several lanes, and the inside test meets the hull's own vertices
  if ((ax == bx && ay == by) || (ax == cx && ay == cy) || (bx == cx && by == cy)) return 0;
  return kf_orient_exact(ax, ay, bx, by, cx, cy);
}

// the plain double expression, as a program without the exact path would write it (what the probe's test shows to be wrong)
BA_HD int kf_orient_naive(KfPoint a, KfPoint b, KfPoint c) {
  BA_NO_CONTRACT
  const double det = ((double)b.x - (double)a.x) * ((double)c.y - (double)a.y) - ((double)b.y - (double)a.y) * ((double)c.x - (double)a.x);
  return det > 0 ? 1 : det < 0 ? -1 : 0;
}

BA_HD bool kf_same(KfPoint p, KfPoint q) { return p.x == q.x && p.y == q.y; }  // -0 = +0, as over the rationals

// q lies beyond p on the ray from c through p (c, p, q collinear, p and q on the same side of c, p != c): comparisons only
BA_HD bool kf_beyond(KfPoint c, KfPoint p, KfPoint q) {
  if (p.x != c.x) return p.x > c.x ? q.x > p.x : q.x < p.x;
  return p.y > c.y ? q.y > p.y : q.y < p.y;
}

// a candidate for the next hull vertex: index (-1 = none) and coordinates
struct KfCand { int idx; KfPoint p; };

// the better of two candidates for the vertex after c on the counter-clockwise hull: the one more clockwise as seen from c; of
// two on one ray the farther; of two with equal coordinates the lower index.  Symmetric: kf_pick(c, p, q) = kf_pick(c, q, p).
BA_HD KfCand kf_pick(KfPoint c, KfCand p, KfCand q) {
  if (q.idx < 0) return p;
  if (p.idx < 0) return q;
  const int s = kf_orient_sign(c, p.p, q.p);
  if (s != 0) return s < 0 ? q : p;
  if (kf_beyond(c, p.p, q.p)) return q;
  if (kf_beyond(c, q.p, p.p)) return p;
  return q.idx < p.idx ? q : p;
}

// the lowest point: smallest y, then smallest x, then lowest index
BA_HD KfCand kf_lowest(KfCand p, KfCand q) {
  if (q.idx < 0) return p;
  if (p.idx < 0) return q;
  if (q.p.y != p.p.y) return q.p.y < p.p.y ? q : p;
  if (q.p.x != p.p.x) return q.p.x < p.p.x ? q : p;
  return q.idx < p.idx ? q : p;
}

// the shoelace sum over hull[0..h) in order, and the area; h < 3 has area 0 by definition (the rounded sum of a degenerate hull
// need not cancel)
BA_HD double kf_shoelace(const KfPoint* pts, const int32_t* hull, int h) {
  BA_NO_CONTRACT
  if (h < 3) return 0.0;
  double a = 0.0;
  KfPoint prev = pts[hull[h - 1]];
  for (int i = 0; i < h; ++i) {
    const KfPoint p = pts[hull[i]];
    const double t = (double)prev.x * (double)p.y - (double)prev.y * (double)p.x;
    a = a + t;
    prev = p;
  }
  return fabs(a * 0.5);
}

// one image's results
struct KfRecord {
  double area_all, area_matched;
  int32_t n_matched, hull_all_size, hull_matched_size, n_inside;
  int32_t flags, reserved;
};

// Frontend.cpp:307-368 on the records of a job's images, in camera order.  std::max(a, b) is (a < b) ? b : a: a NaN overlapArea
// replaces the running value, and the next image replaces the NaN.
inline int kf_fold(const KfRecord* rec, int n_cams, int num_frames, int initialized, float thr_overlap, float thr_ratio, double* overlap_out,
                   double* ratio_out) {
  double overlap = 0.0, ratio = 0.0;
  for (int im = 0; im < n_cams; ++im) {
    const KfRecord& R = rec[im];
    if (R.flags & (KF_FEW_POINTS | KF_FEW_MATCHES)) continue;
    const double overlapArea = R.area_matched / R.area_all;
    const double matchingRatio = (double)R.n_matched / (double)R.n_inside;
    overlap = (overlapArea < overlap) ? overlap : overlapArea;
    ratio = (matchingRatio < ratio) ? ratio : matchingRatio;
  }
  *overlap_out = overlap, *ratio_out = ratio;
  if (num_frames < 2) return 1;
  if (!initialized) return 0;
  return !(overlap > (double)thr_overlap && ratio > (double)thr_ratio);
}

// The gift wrapping as a plain loop: the hull of the points with use[k] != 0 (use = nullptr: of all).  -> the size; hull[0..size)
inline int kf_hull_serial(const KfPoint* pts, const uint8_t* use, int n, int32_t* hull) {
  KfCand v0{-1, {0, 0}};
  for (int k = 0; k < n; ++k)
    if (!use || use[k]) v0 = kf_lowest(v0, KfCand{k, pts[k]});
  if (v0.idx < 0) return 0;
  int h = 0;
  KfCand cur = v0;
  do {
    hull[h++] = cur.idx;
    KfCand best{-1, {0, 0}};
    for (int k = 0; k < n; ++k)
      if ((!use || use[k]) && !kf_same(pts[k], cur.p)) best = kf_pick(cur.p, best, KfCand{k, pts[k]});
    cur = best;
  } while (cur.idx >= 0 && !kf_same(cur.p, v0.p) && h < n);
  return h;
}

// the per-image statement as a plain loop; hull_all / hull_matched have room for n entries each
inline KfRecord kf_image_serial(const KfPoint* pts, const uint8_t* matched, int n, int32_t* hull_all, int32_t* hull_matched) {
  KfRecord R = {0.0, 0.0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < n; ++k) R.n_matched += matched[k] != 0;
  if (n < 3) { R.flags = KF_FEW_POINTS; return R; }
  if (R.n_matched < 3) { R.flags = KF_FEW_MATCHES; return R; }
  R.hull_all_size = kf_hull_serial(pts, nullptr, n, hull_all);
  R.hull_matched_size = kf_hull_serial(pts, matched, n, hull_matched);
  R.area_all = kf_shoelace(pts, hull_all, R.hull_all_size);
  R.area_matched = kf_shoelace(pts, hull_matched, R.hull_matched_size);
  const int h = R.hull_matched_size;
  if (h >= 3)
    for (int k = 0; k < n; ++k) {
      bool in = true;
      for (int i = 0; i < h && in; ++i) in = kf_orient_sign(pts[hull_matched[i]], pts[hull_matched[i + 1 < h ? i + 1 : 0]], pts[k]) > 0;
      R.n_inside += in;
    }
  return R;
}

#if defined(__HIPCC__)
struct KfImage {
  int32_t kp_begin, n;  // keypoints kp_begin .. kp_begin + n - 1 of the pool
  int32_t hull0;        // where the image's two hull lists start (room for n entries each)
  int32_t reserved;
};
struct KfParams {
  const KfPoint* xy;       // [n_kp] the pool's coordinates
  const uint8_t* matched;  // [n_kp]
  const KfImage* images;
  KfRecord* rec;           // [n_images]
  int32_t* hull_all;       // [sum n]
  int32_t* hull_matched;
};

constexpr int KF_THREADS = 64;  // one wave per workgroup

// the LDS of a wave is written and read by that wave only: order the two within the wave
__device__ __forceinline__ void kf_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ KfCand kf_shfl_xor(KfCand c, int mask) {
  KfCand o;
  o.idx = __shfl_xor(c.idx, mask, 64);
  o.p.x = __shfl_xor(c.p.x, mask, 64);
  o.p.y = __shfl_xor(c.p.y, mask, 64);
  return o;
}

// which of a lane's keypoints are matched: bit j of the pair stands for keypoint lane + 64 j (at most 128 of them per lane)
struct KfMask {
  unsigned long long lo, hi;
  __device__ __forceinline__ void set(int j) { (j < 64 ? lo : hi) |= 1ull << (j & 63); }
  __device__ __forceinline__ bool test(int j) const { return ((j < 64 ? lo : hi) >> (j & 63)) & 1ull; }
};
static_assert(KF_MAX_KEYPOINTS <= 64 * 128, "a lane's share of the keypoints fits the two mask words");

// the hull of pts[k], k in [0, n), restricted to the lane's masked keypoints under USE: the hull's indices to hull[], stored by
// every lane alike; -> the size.  The scans read LDS and registers only.
template <bool USE>
__device__ int kf_hull_wave(const KfPoint* pts, const KfMask use, int n, int lane, int32_t* hull) {
  KfCand v0{-1, {0.f, 0.f}};
  for (int k = lane, j = 0; k < n; k += 64, ++j)
    if (!USE || use.test(j)) v0 = kf_lowest(v0, KfCand{k, pts[k]});
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v0 = kf_lowest(v0, kf_shfl_xor(v0, m));
  if (v0.idx < 0) return 0;
  int h = 0;
  KfCand cur = v0;
  do {
    hull[h++] = cur.idx;  // the same value from every lane: each lane reads back its own store
    KfCand best{-1, {0.f, 0.f}};
    for (int k = lane, j = 0; k < n; k += 64, ++j) {
      if (USE && !use.test(j)) continue;
      const KfPoint p = pts[k];
      if (!kf_same(p, cur.p)) best = kf_pick(cur.p, best, KfCand{k, p});
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) best = kf_pick(cur.p, best, kf_shfl_xor(best, m));
    cur = best;
  } while (cur.idx >= 0 && !kf_same(cur.p, v0.p) && h < n);
  return h;
}

// A wave walking a hull's vertices j0, j0 + 1, ... upwards (vertex h is vertex 0 again): the lanes fetch 64 vertices at a time,
// lane l the vertex l places ahead, and hand them out by shuffle.  at() is called by the whole wave, for consecutive j.
struct KfHullWalk {
  const KfPoint* pts;
  const int32_t* hull;
  int h, lane, j0;
  KfPoint held;
  __device__ __forceinline__ KfPoint at(int j) {
    const int slot = (j - j0) & 63;
    if (slot == 0) {
      const int t = j + lane;
      held = pts[hull[t < h ? t : 0]];
    }
    return KfPoint{__shfl(held.x, slot, 64), __shfl(held.y, slot, 64)};
  }
};

// kf_shoelace by a wave: the same operations in the same order, every lane computing the same sum
__device__ double kf_shoelace_wave(const KfPoint* pts, const int32_t* hull, int h, int lane) {
  BA_NO_CONTRACT
  if (h < 3) return 0.0;
  KfHullWalk walk{pts, hull, h, lane, 0, {0.f, 0.f}};
  double a = 0.0;
  KfPoint prev = pts[hull[h - 1]];
  for (int i = 0; i < h; ++i) {
    const KfPoint p = walk.at(i);
    const double t = (double)prev.x * (double)p.y - (double)prev.y * (double)p.x;
    a = a + t;
    prev = p;
  }
  return fabs(a * 0.5);
}

__global__ void __launch_bounds__(KF_THREADS) keyframe_kernel(const KfParams P) {
  extern __shared__ KfPoint kf_lds[];  // [the largest n of the call]
  KfPoint* const kf_pts = kf_lds;
  const int lane = threadIdx.x;
  const KfImage im = P.images[blockIdx.x];
  const int n = im.n;
  const KfPoint* xy = P.xy + im.kp_begin;
  const uint8_t* matched = P.matched + im.kp_begin;
  KfMask mask{0ull, 0ull};
  int m = 0;
  for (int k = lane, j = 0; k < n; k += 64, ++j) {
    kf_pts[k] = xy[k];
    if (matched[k]) mask.set(j), ++m;
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) m += __shfl_xor(m, s, 64);
  kf_wave_sync();
  KfRecord R = {0.0, 0.0, m, 0, 0, 0, 0, 0};
  if (n < 3) {
    R.flags = KF_FEW_POINTS;
  } else if (m < 3) {
    R.flags = KF_FEW_MATCHES;
  } else {
    int32_t* hull_all = P.hull_all + im.hull0;
    int32_t* hull_m = P.hull_matched + im.hull0;
    R.hull_all_size = kf_hull_wave<false>(kf_pts, mask, n, lane, hull_all);
    R.hull_matched_size = kf_hull_wave<true>(kf_pts, mask, n, lane, hull_m);
    R.area_all = kf_shoelace_wave(kf_pts, hull_all, R.hull_all_size, lane);
    R.area_matched = kf_shoelace_wave(kf_pts, hull_m, R.hull_matched_size, lane);
    const int h = R.hull_matched_size;
    if (h >= 3) {
      int inside = 0;
      const KfPoint first = kf_pts[hull_m[0]];
      for (int base = 0; base < n; base += 64) {
        const int k = base + lane;
        bool in = k < n;
        const KfPoint p = kf_pts[in ? k : 0];
        KfHullWalk walk{kf_pts, hull_m, h, lane, 1, {0.f, 0.f}};
        KfPoint a = first;
        for (int j = 1; j <= h && __ballot(in) != 0ull; ++j) {  // the edge from vertex j - 1 to vertex j
          const KfPoint b = walk.at(j);
          if (in) in = kf_orient_sign(a, b, p) > 0;
          a = b;
        }
        inside += __popcll(__ballot(in));
      }
      R.n_inside = inside;
    }
  }
  if (lane == 0) P.rec[blockIdx.x] = R;
}
#endif  // __HIPCC__

}  // namespace fe
