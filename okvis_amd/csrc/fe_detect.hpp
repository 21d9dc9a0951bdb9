// Keypoint detection of the OKVIS frontend on the device (include/okvis_amd_frontend.h: okvis_fe_detect_keypoints): what
// Frontend::detectAndDescribe (okvis_frontend/src/Frontend.cpp:92-114) asks of its detector under the shipped configuration
// (octaves 0: one scale at full resolution) — a Harris score on the 8-bit image, a 3 x 3 maximum search above an absolute
// threshold, and a selection of the strongest maxima that keeps them apart — for many images per call.
//
// The reference's detector is brisk::ScaleSpaceFeatureDetector<brisk::HarrisScoreCalculator>, and BRISK's source is not part of
// the reference tree: the detector is stated in the header from its definition and is NOT pinned to BRISK.  Images are 8-bit, so
// the statement is integer arithmetic and exact; the two sub-pixel offsets are one IEEE division and one addition each.
//
//   det_sobel        Ix, Iy of one pixel from its 3 x 3 neighbourhood, |Ix|, |Iy| <= 1020: a pair of int16
//   det_score        S = 16 (A C - B^2) - (A + C)^2 from the 3 x 3 neighbourhood of gradients under the binomial weights.
//                    A, C <= 16 * 1020^2 = 16 646 400 and |B| likewise: int32 sums; A C <= 2.78e14, |S| < 5.6e15 < 2^53: int64
//   det_beats        the total order "larger S, then lower row-major index" on (S, key) with key = y << 16 | x
//   det_offset       the parabola's vertex through three scores, clamped to [-0.5, 0.5]
//   det_close        integer squared distance of two keys below min_dist^2
//   DetOrder         what a selection asks of its candidates: the key type, load, beats, close, accept.  The scale space has its
//                    own (DetScaledOrder of fe_detect_scale.hpp); the selection itself is written once per side:
//   det_select_serial    (host) ORDERS the candidates by the order's beats and walks them, where det_select_rounds (device) takes
//                    the strongest remaining one by reduction; both give the statement's result because the order is total
//   det_layer_candidates_serial, detect_image_serial   the candidates of one image, and the whole per-image statement, as plain
//                    loops (host referee of the probe, CPU side of the benchmark)
//
// detect_score_kernel: one workgroup of 256 lanes per DET_TILE_X x DET_TILE_Y tile of one image (a tile table built on the host).
// The tile's bytes go to LDS with a halo of 3 (one pixel for Sobel, one for the window, one for the neighbour test; coordinates
// clamped to the image, what the clamped pixels feed lies outside the score domain), then the packed gradients with a halo of 2,
// then the scores with a halo of 1 (DET_OUTSIDE beyond the score domain: beaten by every candidate).  Only candidates leave the
// tile: one 24-byte record each, appended to the image's list through one atomic counter per image.  The list's order in memory
// is whatever the hardware made it; nothing downstream reads it as an order.  The score image goes to memory only for a referee.
//
// detect_select_kernel: one workgroup of 1024 lanes per image: the overflow rule, then det_select_rounds under DetOrder.
// det_select_rounds: lane t holds candidates t, t + 1024, ... (at most 8: the limit of 8192) as (S, key) in registers; one out of
// play has S = 0.  Per accepted keypoint: every lane's best in play, a 6-step butterfly per wave, the sixteen waves' results
// through LDS (two buffers in turn: one barrier per keypoint) and a 4-step butterfly, then every lane strikes out what lies inside
// the winner's disc.  At most max_keypoints + 1 rounds; no scratch, no atomics.  The key type is the order's (32 bits here, 64
// over a scale space): the one-layer kernel keeps its registers and shuffles.
//
// The per-pixel and per-candidate functions are BA_HD like ba_math.hpp's: a plain host compiler sees them too.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "ba_math.hpp"

namespace fe {

constexpr int DET_TILE_X = 64, DET_TILE_Y = 16;  // the score kernel's tile; okvis_amd/frontend.py holds the same two numbers
constexpr int DET_MIN_DIM = 5, DET_MAX_DIM = 8192;
constexpr int DET_MAX_KEYPOINTS = 2048;
constexpr int DET_SEL_THREADS = 1024, DET_SEL_PER_LANE = 8;
constexpr int DET_MAX_CANDIDATES = DET_SEL_THREADS * DET_SEL_PER_LANE;  // 8192: what the selection kernel holds in registers
constexpr int DET_OVERFLOW = 1, DET_FULL = 2;                           // OKVIS_FE_DETECT_*
constexpr int64_t DET_OUTSIDE = INT64_MIN;                              // a score beyond the score domain
static_assert(DET_MAX_DIM <= 65536, "x and y share one 32-bit key");

struct DetCand {  // a candidate, and a selected keypoint
  int64_t s;
  int32_t x, y;   // the integer maximum
  float fx, fy;   // the sub-pixel position
};
static_assert(sizeof(DetCand) == 24, "layout");

struct DetResult { int32_t n_keypoints, n_candidates, flags, reserved; };

// r0, r1, r2 point at column x - 1 of the rows y - 1, y, y + 1 -> Ix | Iy << 16 as two int16
BA_HD uint32_t det_sobel(const uint8_t* r0, const uint8_t* r1, const uint8_t* r2) {
  const int32_t ix = ((int32_t)r0[2] + 2 * (int32_t)r1[2] + (int32_t)r2[2]) - ((int32_t)r0[0] + 2 * (int32_t)r1[0] + (int32_t)r2[0]);
  const int32_t iy = ((int32_t)r2[0] + 2 * (int32_t)r2[1] + (int32_t)r2[2]) - ((int32_t)r0[0] + 2 * (int32_t)r0[1] + (int32_t)r0[2]);
  return ((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16);
}
BA_HD int32_t det_ix(uint32_t g) { return (int32_t)(int16_t)(uint16_t)(g & 0xffffu); }
BA_HD int32_t det_iy(uint32_t g) { return (int32_t)(int16_t)(uint16_t)(g >> 16); }

// g points at the packed gradient of (x - 1, y - 1), rows `stride` entries apart
BA_HD int64_t det_score(const uint32_t* g, int stride) {
  int32_t a = 0, b = 0, c = 0;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int32_t k = (dx == 1 ? 2 : 1) * (dy == 1 ? 2 : 1);
      const uint32_t v = g[dy * stride + dx];
      const int32_t ix = det_ix(v), iy = det_iy(v);
      a += k * ix * ix, b += k * ix * iy, c += k * iy * iy;
    }
  const int64_t A = a, B = b, C = c;
  return 16 * (A * C - B * B) - (A + C) * (A + C);
}

BA_HD uint32_t det_key(int32_t x, int32_t y) { return ((uint32_t)y << 16) | (uint32_t)x; }
BA_HD int32_t det_key_x(uint32_t k) { return (int32_t)(k & 0xffffu); }
BA_HD int32_t det_key_y(uint32_t k) { return (int32_t)(k >> 16); }

// p beats q: x < width <= 65536, so the order of the keys is the order of y * width + x
BA_HD bool det_beats(int64_t sp, uint32_t kp, int64_t sq, uint32_t kq) { return sp > sq || (sp == sq && kp < kq); }

// sm, s0, sp: the scores at -1, 0, +1 along one axis (a neighbour beyond the domain already replaced by s0)
BA_HD double det_offset(int64_t sm, int64_t s0, int64_t sp) {
  BA_NO_CONTRACT
  const int64_t num = sm - sp, den = 2 * (sm - 2 * s0 + sp);
  if (den == 0) return 0.0;
  const double d = (double)num / (double)den;
  return d < -0.5 ? -0.5 : (d > 0.5 ? 0.5 : d);
}
BA_HD float det_position(int32_t x, double d) {
  BA_NO_CONTRACT
  return (float)((double)x + d);
}

// the candidate at (x, y) with score s from its four axis neighbours (DET_OUTSIDE beyond the domain)
BA_HD DetCand det_candidate(int32_t x, int32_t y, int64_t s, int64_t left, int64_t right, int64_t up, int64_t down) {
  DetCand c;
  c.s = s, c.x = x, c.y = y;
  c.fx = det_position(x, det_offset(left == DET_OUTSIDE ? s : left, s, right == DET_OUTSIDE ? s : right));
  c.fy = det_position(y, det_offset(up == DET_OUTSIDE ? s : up, s, down == DET_OUTSIDE ? s : down));
  return c;
}

// squared distances stay below 2 * 65535^2 < 2^33
BA_HD bool det_close(uint32_t ka, uint32_t kb, int64_t min_dist2) {
  const int64_t dx = det_key_x(ka) - det_key_x(kb), dy = det_key_y(ka) - det_key_y(kb);
  return dx * dx + dy * dy < min_dist2;
}

// The selection's order over one-layer candidates, for det_select_rounds (the device) and det_select_serial (the host) alike.
// An order names its Key and supplies load (candidate i as (S, key)), beats (the total order), close (two keys nearer than the
// job's minimum distance) and accept (candidate pos becomes keypoint number slot).
struct DetOrder {
  using Key = uint32_t;
  const DetCand* cand;  // the job's candidates
  DetCand* sel;         // the job's keypoints
  int64_t min_dist2;
  BA_HD void load(int i, int64_t& s, Key& k) const { s = cand[i].s, k = det_key(cand[i].x, cand[i].y); }
  BA_HD static bool beats(int64_t sp, Key kp, int64_t sq, Key kq) { return det_beats(sp, kp, sq, kq); }
  BA_HD bool close(Key a, Key b) const { return det_close(a, b, min_dist2); }
  BA_HD void accept(int slot, int pos) const { sel[slot] = cand[pos]; }
};

// The selection as plain loops: the n candidates ORDERED by the order and walked, each accepted unless it lies close to one
// accepted before it; FULL when one more than max_kp would have been accepted.  -> the number accepted
template <class Order>
inline int det_select_serial(const Order& o, int n, int max_kp, int32_t& flags) {
  using Key = typename Order::Key;
  std::vector<int64_t> s((size_t)n);
  std::vector<Key> k((size_t)n), taken;
  std::vector<int32_t> order((size_t)n);
  for (int i = 0; i < n; ++i) o.load(i, s[i], k[i]), order[i] = i;
  std::sort(order.begin(), order.end(), [&](int32_t p, int32_t q) { return Order::beats(s[p], k[p], s[q], k[q]); });
  for (int32_t i : order) {
    bool ok = true;
    for (size_t a = 0; a < taken.size() && ok; ++a) ok = !o.close(k[i], taken[a]);
    if (!ok) continue;
    if ((int)taken.size() == max_kp) {  // one more would have been accepted: the list is cut short
      flags |= DET_FULL;
      break;
    }
    o.accept((int)taken.size(), i);
    taken.push_back(k[i]);
  }
  return (int)taken.size();
}

// the candidates of one w x h layer: S gets the scores, DET_OUTSIDE beyond the domain
inline void det_layer_candidates_serial(const uint8_t* image, int w, int h, int64_t pitch, int64_t threshold, std::vector<int64_t>& S,
                                        std::vector<DetCand>& cand) {
  std::vector<uint32_t> g((size_t)w * h, 0u);
  S.assign((size_t)w * h, DET_OUTSIDE);
  for (int y = 1; y <= h - 2; ++y)
    for (int x = 1; x <= w - 2; ++x) {
      const uint8_t* r = image + (size_t)(y - 1) * pitch + (x - 1);
      g[(size_t)y * w + x] = det_sobel(r, r + pitch, r + 2 * (size_t)pitch);
    }
  for (int y = 2; y <= h - 3; ++y)
    for (int x = 2; x <= w - 3; ++x) S[(size_t)y * w + x] = det_score(&g[(size_t)(y - 1) * w + (x - 1)], w);
  for (int y = 2; y <= h - 3; ++y)
    for (int x = 2; x <= w - 3; ++x) {
      const int64_t s = S[(size_t)y * w + x];
      if (s < threshold) continue;
      bool best = true;
      for (int dy = -1; dy <= 1 && best; ++dy)
        for (int dx = -1; dx <= 1 && best; ++dx)
          if (dx || dy) best = det_beats(s, det_key(x, y), S[(size_t)(y + dy) * w + (x + dx)], det_key(x + dx, y + dy));
      if (best)
        cand.push_back(det_candidate(x, y, s, S[(size_t)y * w + x - 1], S[(size_t)y * w + x + 1], S[(size_t)(y - 1) * w + x],
                                     S[(size_t)(y + 1) * w + x]));
    }
}

// The per-image statement as plain loops.  sel has room for max_keypoints records; score (h * w, or nullptr) receives the score
// image, 0 outside its domain.
inline DetResult detect_image_serial(const uint8_t* image, int w, int h, int pitch, int64_t threshold, int min_dist, int max_keypoints,
                                     int cand_capacity, DetCand* sel, int64_t* score) {
  std::vector<int64_t> S;
  std::vector<DetCand> cand;
  det_layer_candidates_serial(image, w, h, pitch, threshold, S, cand);
  if (score)
    for (size_t i = 0; i < S.size(); ++i) score[i] = S[i] == DET_OUTSIDE ? 0 : S[i];
  DetResult R = {0, (int32_t)cand.size(), 0, 0};
  if ((int64_t)cand.size() > cand_capacity)
    R.flags = DET_OVERFLOW;
  else
    R.n_keypoints = det_select_serial(DetOrder{cand.data(), sel, (int64_t)min_dist * min_dist}, (int)cand.size(), max_keypoints, R.flags);
  return R;
}

#if defined(__HIPCC__)
struct DetImage {  // one job as the device sees it
  int64_t threshold;
  int64_t pix;    // where its bytes start in the pixel pool (rows packed, no pitch)
  int64_t score;  // where its score image starts in the score pool, -1: not asked for
  int32_t w, h;
  int32_t cand0, cap;     // its candidate list: records cand0 .. cand0 + cap - 1
  int32_t sel0, max_kp;   // its selected keypoints: records sel0 .. sel0 + max_kp - 1
  int32_t min_dist, reserved;
};
struct DetTile { int32_t job, x0, y0, reserved; };
struct DetParams {
  const uint8_t* pix;
  const DetImage* images;
  const DetTile* tiles;
  int32_t* count;  // [n_jobs] candidates found, zero on entry
  DetCand* cand;
  DetCand* sel;
  DetResult* res;  // [n_jobs]
  int64_t* score;
};

constexpr int DET_THREADS = 256;
constexpr int DET_PW = DET_TILE_X + 6, DET_PH = DET_TILE_Y + 6;  // pixels: halo 3
constexpr int DET_GW = DET_TILE_X + 4, DET_GH = DET_TILE_Y + 4;  // gradients: halo 2
constexpr int DET_SW = DET_TILE_X + 2, DET_SH = DET_TILE_Y + 2;  // scores: halo 1
constexpr int DET_PSTRIDE = (DET_PW + 3) & ~3;

__global__ void __launch_bounds__(DET_THREADS) detect_score_kernel(const DetParams P) {
  __shared__ uint8_t pix[DET_PH * DET_PSTRIDE];
  __shared__ uint32_t grad[DET_GH * DET_GW];
  __shared__ int64_t sc[DET_SH * DET_SW];
  const int tid = threadIdx.x;
  const DetTile tile = P.tiles[blockIdx.x];
  const DetImage im = P.images[tile.job];
  const int w = im.w, h = im.h, x0 = tile.x0, y0 = tile.y0;
  const uint8_t* src = P.pix + im.pix;
  // LDS pixel (px, py) is image pixel (x0 - 3 + px, y0 - 3 + py), clamped to the image
  for (int i = tid; i < DET_PH * DET_PW; i += DET_THREADS) {
    const int py = i / DET_PW, px = i - py * DET_PW;
    int x = x0 - 3 + px, y = y0 - 3 + py;
    x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x), y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
    pix[py * DET_PSTRIDE + px] = src[(int64_t)y * w + x];
  }
  __syncthreads();
  // LDS gradient (gx, gy) is that of image pixel (x0 - 2 + gx, y0 - 2 + gy): LDS pixels gx .. gx + 2 of rows gy .. gy + 2
  for (int i = tid; i < DET_GH * DET_GW; i += DET_THREADS) {
    const int gy = i / DET_GW, gx = i - gy * DET_GW;
    const uint8_t* r = pix + gy * DET_PSTRIDE + gx;
    grad[i] = det_sobel(r, r + DET_PSTRIDE, r + 2 * DET_PSTRIDE);
  }
  __syncthreads();
  // LDS score (sx, sy) is that of image pixel (x0 - 1 + sx, y0 - 1 + sy): LDS gradients sx .. sx + 2 of rows sy .. sy + 2
  for (int i = tid; i < DET_SH * DET_SW; i += DET_THREADS) {
    const int sy = i / DET_SW, sx = i - sy * DET_SW;
    const int x = x0 - 1 + sx, y = y0 - 1 + sy;
    const bool in = x >= 2 && x <= w - 3 && y >= 2 && y <= h - 3;
    sc[i] = in ? det_score(grad + sy * DET_GW + sx, DET_GW) : DET_OUTSIDE;
  }
  __syncthreads();
  // tile pixel (tx, ty) is image pixel (x0 + tx, y0 + ty) and LDS score (tx + 1, ty + 1)
  for (int i = tid; i < DET_TILE_X * DET_TILE_Y; i += DET_THREADS) {
    const int ty = i / DET_TILE_X, tx = i - ty * DET_TILE_X;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= w || y >= h) continue;
    const int64_t* at = sc + (ty + 1) * DET_SW + (tx + 1);
    const int64_t s = *at;
    if (im.score >= 0) P.score[im.score + (int64_t)y * w + x] = s == DET_OUTSIDE ? 0 : s;
    if (s == DET_OUTSIDE || s < im.threshold) continue;
    bool best = true;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx)
        if (dx || dy) best = best && det_beats(s, det_key(x, y), at[dy * DET_SW + dx], det_key(x + dx, y + dy));
    if (!best) continue;
    const DetCand c = det_candidate(x, y, s, at[-1], at[1], at[-DET_SW], at[DET_SW]);
    const int slot = atomicAdd(P.count + tile.job, 1);  // the true count, past the capacity too
    if (slot < im.cap) P.cand[im.cand0 + slot] = c;
  }
}

// The selection of one workgroup of DET_SEL_THREADS lanes over the n <= DET_MAX_CANDIDATES candidates of an order (DetOrder's
// comment), the body of both selection kernels: the register-resident slots, the rounds, the LDS hand-off and the FULL rule.
// -> the number accepted, the same in every lane
template <class Order>
__device__ __forceinline__ int det_select_rounds(const Order& o, int n, int max_kp, int32_t& flags) {
  using Key = typename Order::Key;
  constexpr int WAVES = DET_SEL_THREADS / 64;
  static_assert(WAVES <= 64 && (WAVES & (WAVES - 1)) == 0, "the waves' results are reduced by one butterfly");
  __shared__ int64_t red_s[2][WAVES];
  __shared__ Key red_k[2][WAVES];
  __shared__ int32_t red_p[2][WAVES];
  const int tid = threadIdx.x;
  // a candidate out of play, and a slot without one, has S = 0 and key 0: it beats nothing, and every candidate (S >= 1) beats it
  int64_t s[DET_SEL_PER_LANE];
  Key k[DET_SEL_PER_LANE];
#pragma unroll
  for (int j = 0; j < DET_SEL_PER_LANE; ++j) {
    const int pos = tid + j * DET_SEL_THREADS;
    const bool in = pos < n;
    int64_t cs;
    Key ck;
    o.load(in ? pos : 0, cs, ck);  // record 0 exists (cap >= 1); what it holds when n = 0 is not used
    s[j] = in ? cs : 0, k[j] = in ? ck : (Key)0;
  }
  int accepted = 0;
#pragma nounroll
  for (int it = 0; it <= max_kp; ++it) {
    // the strongest of the lane's candidates in play, then of the wave's
    int64_t bs = 0;
    Key bk = 0;
    int32_t bp = -1;
#pragma unroll
    for (int j = 0; j < DET_SEL_PER_LANE; ++j) {
      const bool b = Order::beats(s[j], k[j], bs, bk);
      bs = b ? s[j] : bs, bk = b ? k[j] : bk, bp = b ? tid + j * DET_SEL_THREADS : bp;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const int64_t os = __shfl_xor(bs, m, 64);
      const Key ok = __shfl_xor(bk, m, 64);
      const int32_t op = __shfl_xor(bp, m, 64);
      if (Order::beats(os, ok, bs, bk)) bs = os, bk = ok, bp = op;
    }
    const int buf = it & 1;
    if ((tid & 63) == 0) red_s[buf][tid >> 6] = bs, red_k[buf][tid >> 6] = bk, red_p[buf][tid >> 6] = bp;
    __syncthreads();  // one per round: round it + 1 writes the other buffer, round it + 2 comes after the next barrier
    // of the workgroup's: lane l takes wave (l mod WAVES)'s result, log2(WAVES) more steps leave the same winner in every lane
    bs = red_s[buf][tid & (WAVES - 1)], bk = red_k[buf][tid & (WAVES - 1)], bp = red_p[buf][tid & (WAVES - 1)];
#pragma unroll
    for (int m = 1; m < WAVES; m <<= 1) {
      const int64_t os = __shfl_xor(bs, m, 64);
      const Key ok = __shfl_xor(bk, m, 64);
      const int32_t op = __shfl_xor(bp, m, 64);
      if (Order::beats(os, ok, bs, bk)) bs = os, bk = ok, bp = op;
    }
    if (bp < 0) break;  // nothing left in play
    if (accepted == max_kp) {
      flags |= DET_FULL;
      break;
    }
    if (tid == 0) o.accept(accepted, bp);
    ++accepted;
#pragma unroll
    for (int j = 0; j < DET_SEL_PER_LANE; ++j) {
      const bool out = tid + j * DET_SEL_THREADS == bp || o.close(k[j], bk);
      s[j] = out ? 0 : s[j], k[j] = out ? (Key)0 : k[j];
    }
  }
  return accepted;
}

__global__ void __launch_bounds__(DET_SEL_THREADS) detect_select_kernel(const DetParams P) {
  const int job = blockIdx.x;
  const DetImage im = P.images[job];
  const int n = P.count[job];
  DetResult R = {0, n, 0, 0};
  if (n > im.cap)  // the same for every lane
    R.flags = DET_OVERFLOW;
  else
    R.n_keypoints = det_select_rounds(DetOrder{P.cand + im.cand0, P.sel + im.sel0, (int64_t)im.min_dist * im.min_dist}, n, im.max_kp, R.flags);
  if (threadIdx.x == 0) P.res[job] = R;
}
#endif  // __HIPCC__

}  // namespace fe
