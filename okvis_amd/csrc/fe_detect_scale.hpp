// Keypoint detection over a scale space on the device (include/okvis_amd_frontend.h: okvis_fe_detect_keypoints_scaled,
// okvis_fe_detect_scaled_and_describe): the detector of fe_detect.hpp on every layer of a half-sampled pyramid (the reference's
// detection option `octaves` > 0), a comparison of raw Harris scores across neighbouring layers, a scale per keypoint that goes
// into its size, and one selection over the survivors of all layers.
//
// Like the detector itself the scale space is stated in the header from its definition and is NOT pinned to BRISK: no
// intra-octaves, a raw score comparison across layers, a linear scale interpolation.  Everything is integer arithmetic but the
// scale and the positions, which are a handful of IEEE operations without a fused multiply-add.
//
//   det_layers           the layers of an image: w, h halved while both stay >= 5, at most octaves + 1 of them
//   det_half             one pixel of layer l + 1 from its four of layer l
//   det_patch<N>         the scores of N x N pixels recomputed from (N + 4)^2 pixels (DET_OUTSIDE beyond the score domain)
//   det_below, det_above the maxima s_m, s_p of the two footprints in the neighbouring layers
//   det_survives         S > s_m (the finer layer wins a tie) and S >= s_p
//   det_scale, det_scaled_size, det_scaled_position   t 2^l, the size and the full-resolution position
//   det_scaled_beats     the order "larger S, then lower layer, then lower row-major index" on (S, layer << 32 | y << 16 | x)
//   det_scaled_close     squared distance of two centres in doubled full-resolution units below 4 min_dist^2
//   DetScaledOrder       these three as an order of the selection (fe_detect.hpp: det_select_rounds, det_select_serial)
//   detect_scaled_image_serial   the whole per-image statement as plain loops (host referee of the probe, CPU side of the benchmark)
//
// detect_pyramid_kernel: one workgroup of 256 lanes per 64 x 16 tile of layer 0 (of the jobs with more than one layer).  Every
// descendant of a tile's pixels lies in the tile (32 x 8, 16 x 4, 8 x 2, 4 x 1), so the tile goes through all layers in LDS with
// one barrier per layer and every layer's pixels are written behind the images in the pixel pool.
// The unchanged detect_score_kernel then takes every (job, layer) as one more image of its tile table.
// detect_cross_kernel: one workgroup per (job, layer); lane t takes the layer's candidates t, t + 256, ... up to min(count, cap).
// The 16 + 9 scores of the neighbouring layers (and the four axis neighbours of a candidate above layer 0, whose sub-pixel offset
// is needed in double) are recomputed from pool pixels; a survivor is appended to the job's pooled list through one counter per
// job.  The list's order in memory reaches no output.
// detect_select_scaled_kernel: the layers' counts, the overflow rule over all layers, then det_select_rounds under DetScaledOrder
// (the three-level order and the doubled-centre distance) on the job's pooled survivors.
#pragma once
#include "fe_detect.hpp"

namespace fe {

constexpr int DET_MAX_OCTAVES = 4, DET_MAX_LAYERS = DET_MAX_OCTAVES + 1;   // OKVIS_FE_DETECT_MAX_OCTAVES
static_assert((DET_TILE_X >> DET_MAX_OCTAVES) >= 1 && (DET_TILE_Y >> DET_MAX_OCTAVES) >= 1, "a tile of layer 0 holds its descendants in every layer");

struct DetLayers { int32_t n, w[DET_MAX_LAYERS], h[DET_MAX_LAYERS]; };
struct DetScaleExtra {   // what a survivor carries besides its DetCand (whose x, y are in its layer, fx, fy at full resolution)
  double scale;
  float size;
  int32_t layer;
};
static_assert(sizeof(DetScaleExtra) == 16, "layout");

BA_HD DetLayers det_layers(int w, int h, int octaves) {
  DetLayers L;
  L.n = 1, L.w[0] = w, L.h[0] = h;
  for (int l = 1; l < DET_MAX_LAYERS; ++l) L.w[l] = L.h[l] = 0;
  for (int l = 0; l < DET_MAX_OCTAVES; ++l) {
    if (l >= octaves || (L.w[l] >> 1) < DET_MIN_DIM || (L.h[l] >> 1) < DET_MIN_DIM) break;
    L.w[l + 1] = L.w[l] >> 1, L.h[l + 1] = L.h[l] >> 1, L.n = l + 2;
  }
  return L;
}

BA_HD uint8_t det_half(int32_t a, int32_t b, int32_t c, int32_t d) { return (uint8_t)((a + b + c + d + 2) >> 2); }

// most candidates a w x h layer can have: two 8-neighbours never both beat each other, so at most every other pixel of every
// other row of the score domain is one
BA_HD int32_t det_layer_bound(int w, int h) { return ((w - 4 + 1) >> 1) * ((h - 4 + 1) >> 1); }

// The scores of the pixels (x0 + i, y0 + j), 0 <= i, j < N, of a w x h layer (rows `stride` bytes apart) into out[j * N + i],
// DET_OUTSIDE beyond the score domain.  Coordinates are clamped to the layer; a clamped pixel feeds no score of the domain.
template <int N>
BA_HD void det_patch(const uint8_t* pix, int64_t stride, int w, int h, int x0, int y0, int64_t* out) {
  constexpr int PW = N + 4, GW = N + 2;
  uint8_t p[PW * PW];
  uint32_t g[GW * GW];
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    int y = y0 - 2 + j;
    y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
#pragma unroll
    for (int i = 0; i < PW; ++i) {
      int x = x0 - 2 + i;
      x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
      p[j * PW + i] = pix[(int64_t)y * stride + x];
    }
  }
#pragma unroll
  for (int j = 0; j < GW; ++j)
#pragma unroll
    for (int i = 0; i < GW; ++i) g[j * GW + i] = det_sobel(p + j * PW + i, p + (j + 1) * PW + i, p + (j + 2) * PW + i);
#pragma unroll
  for (int j = 0; j < N; ++j)
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int x = x0 + i, y = y0 + j;
      const bool in = x >= 2 && x <= w - 3 && y >= 2 && y <= h - 3;
      out[j * N + i] = in ? det_score(g + j * GW + i, GW) : DET_OUTSIDE;
    }
}

// s_m of the candidate (x, y) of layer l >= 1: the largest of S_{l-1}[2y + j][2x + i], i, j in -1..2.  All 16 lie in the score
// domain of the w x h layer l - 1 (see the header), so the result is a score.
BA_HD int64_t det_below(const uint8_t* fine, int64_t stride, int w, int h, int x, int y) {
  int64_t s[16];
  det_patch<4>(fine, stride, w, h, 2 * x - 1, 2 * y - 1, s);
  int64_t m = s[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) m = s[i] > m ? s[i] : m;
  return m;
}
// s_p of the candidate (x, y) of layer l: the largest of S_{l+1}[(y >> 1) + j][(x >> 1) + i], i, j in -1..1, inside the score
// domain of the w x h layer l + 1; DET_OUTSIDE when none of the nine is (the side counts as missing)
BA_HD int64_t det_above(const uint8_t* coarse, int64_t stride, int w, int h, int x, int y) {
  int64_t s[9];
  det_patch<3>(coarse, stride, w, h, (x >> 1) - 1, (y >> 1) - 1, s);
  int64_t m = s[0];
#pragma unroll
  for (int i = 1; i < 9; ++i) m = s[i] > m ? s[i] : m;
  return m;
}
// the four axis neighbours of (x, y) in its own layer: left, right, up, down (DET_OUTSIDE beyond the domain)
BA_HD void det_axes(const uint8_t* pix, int64_t stride, int w, int h, int x, int y, int64_t* lrud) {
  int64_t s[9];
  det_patch<3>(pix, stride, w, h, x - 1, y - 1, s);
  lrud[0] = s[3], lrud[1] = s[5], lrud[2] = s[1], lrud[3] = s[7];
}

// has_below: l >= 1; has_above: layer l + 1 exists and one of its nine pixels has a score
BA_HD bool det_survives(int64_t s, bool has_below, int64_t sm, bool has_above, int64_t sp) {
  return (!has_below || s > sm) && (!has_above || s >= sp);
}
BA_HD double det_scale(int layer, bool both, int64_t sm, int64_t s, int64_t sp) {
  BA_NO_CONTRACT
  const double d = both ? det_offset(sm, s, sp) : 0.0;
  const double t = d >= 0.0 ? 1.0 + d : 1.0 + 0.5 * d;
  return t * (double)(1 << layer);
}
BA_HD float det_scaled_size(float kp_size, double scale) {
  BA_NO_CONTRACT
  return (float)((double)kp_size * scale);
}
// d: the sub-pixel offset in the layer; layer 0 keeps det_position's expression (octaves = 0 gives the one-layer entry's bytes)
BA_HD float det_scaled_position(int32_t x, double d, int layer) {
  BA_NO_CONTRACT
  const double u = (double)x + d;
  if (layer == 0) return (float)u;
  return (float)((u + 0.5) * (double)(1 << layer) - 0.5);
}

BA_HD uint64_t det_scaled_key(int layer, int32_t x, int32_t y) { return ((uint64_t)layer << 32) | det_key(x, y); }
BA_HD int det_scaled_key_layer(uint64_t k) { return (int)(k >> 32); }
BA_HD bool det_scaled_beats(int64_t sp, uint64_t kp, int64_t sq, uint64_t kq) { return sp > sq || (sp == sq && kp < kq); }
// the centre of pixel x of layer l in doubled full-resolution units: 2 ((x + 0.5) 2^l - 0.5), below 2 * 8192
BA_HD int32_t det_centre(int32_t x, int layer) { return ((2 * x + 1) << layer) - 1; }
// 4 min_dist^2 without leaving int64: no two centres are 2^16 apart, so a min_dist beyond 2^15 closes every pair like 2^15 does
BA_HD int64_t det_scaled_reach(int32_t min_dist) {
  const int64_t m = min_dist > (1 << 15) ? (1 << 15) : min_dist;
  return 4 * m * m;
}
BA_HD bool det_scaled_close(uint64_t ka, uint64_t kb, int64_t reach) {
  const int la = det_scaled_key_layer(ka), lb = det_scaled_key_layer(kb);
  const int64_t dx = det_centre(det_key_x((uint32_t)ka), la) - det_centre(det_key_x((uint32_t)kb), lb);
  const int64_t dy = det_centre(det_key_y((uint32_t)ka), la) - det_centre(det_key_y((uint32_t)kb), lb);
  return dx * dx + dy * dy < reach;
}

struct DetLayerView {   // one layer's pixels
  const uint8_t* pix;
  int64_t stride;   // bytes from row to row
  int32_t w, h;
};
struct DetSurvivor {
  DetCand c;   // x, y in the layer; fx, fy at full resolution
  DetScaleExtra e;
  bool alive;
};

// One layer candidate c of layer l against its neighbouring layers: `fine` is layer l - 1 (read when l >= 1), `own` layer l,
// `coarse` layer l + 1 (read when has_coarse).  Not alive: the rest of the result is not to be read.
BA_HD DetSurvivor det_cross(const DetCand& c, int l, bool has_coarse, const DetLayerView& fine, const DetLayerView& own, const DetLayerView& coarse,
                            float kp_size) {
  DetSurvivor r;
  const bool has_below = l >= 1;
  int64_t sm = DET_OUTSIDE, sp = DET_OUTSIDE;
  if (has_below) sm = det_below(fine.pix, fine.stride, fine.w, fine.h, c.x, c.y);
  if (has_coarse) sp = det_above(coarse.pix, coarse.stride, coarse.w, coarse.h, c.x, c.y);
  const bool has_above = sp != DET_OUTSIDE;
  r.c = c;
  r.alive = det_survives(c.s, has_below, sm, has_above, sp);
  if (r.alive && l >= 1) {   // the offsets again, in double: the candidate holds them added to x and rounded to float
    int64_t a[4];
    det_axes(own.pix, own.stride, own.w, own.h, c.x, c.y, a);
    r.c.fx = det_scaled_position(c.x, det_offset(a[0] == DET_OUTSIDE ? c.s : a[0], c.s, a[1] == DET_OUTSIDE ? c.s : a[1]), l);
    r.c.fy = det_scaled_position(c.y, det_offset(a[2] == DET_OUTSIDE ? c.s : a[2], c.s, a[3] == DET_OUTSIDE ? c.s : a[3]), l);
  }
  r.e.scale = det_scale(l, has_below && has_above, sm, c.s, sp);
  r.e.size = det_scaled_size(kp_size, r.e.scale);
  r.e.layer = l;
  return r;
}

// the selection's order over the pooled survivors of all layers (DetOrder's comment)
struct DetScaledOrder {
  using Key = uint64_t;
  const DetCand* pool;   // the job's survivors
  const DetScaleExtra* poolx;
  DetCand* sel;          // the job's keypoints
  DetScaleExtra* selx;
  int64_t reach;
  BA_HD void load(int i, int64_t& s, Key& k) const { s = pool[i].s, k = det_scaled_key(poolx[i].layer, pool[i].x, pool[i].y); }
  BA_HD static bool beats(int64_t sp, Key kp, int64_t sq, Key kq) { return det_scaled_beats(sp, kp, sq, kq); }
  BA_HD bool close(Key a, Key b) const { return det_scaled_close(a, b, reach); }
  BA_HD void accept(int slot, int pos) const { sel[slot] = pool[pos], selx[slot] = poolx[pos]; }
};

// The per-image statement as plain loops.  sel, selx have room for max_keypoints records; layer_counts for DET_MAX_LAYERS counts;
// score (sum_l h_l w_l, or nullptr) receives the layers' score images one behind the other, 0 outside their domains; pyramid
// (sum_{l >= 1} h_l w_l, or nullptr) the layers 1.. one behind the other.
inline DetResult detect_scaled_image_serial(const uint8_t* image, int w, int h, int pitch, int64_t threshold, int octaves, int min_dist,
                                            int max_keypoints, int cand_capacity, float kp_size, DetCand* sel, DetScaleExtra* selx,
                                            int32_t* n_layers, int32_t* layer_counts, int64_t* score, uint8_t* pyramid) {
  const DetLayers L = det_layers(w, h, octaves);
  *n_layers = L.n;
  std::vector<std::vector<uint8_t>> own((size_t)L.n);
  DetLayerView view[DET_MAX_LAYERS + 1] = {};   // one past the last layer: what det_cross is handed and does not read
  view[0] = DetLayerView{image, pitch, w, h};
  for (int l = 1; l < L.n; ++l) {
    own[l].resize((size_t)L.w[l] * L.h[l]);
    for (int y = 0; y < L.h[l]; ++y)
      for (int x = 0; x < L.w[l]; ++x) {
        const uint8_t* r = view[l - 1].pix + (size_t)(2 * y) * view[l - 1].stride + 2 * x;
        own[l][(size_t)y * L.w[l] + x] = det_half(r[0], r[1], r[view[l - 1].stride], r[view[l - 1].stride + 1]);
      }
    view[l] = DetLayerView{own[l].data(), L.w[l], L.w[l], L.h[l]};
    if (pyramid) pyramid = std::copy(own[l].begin(), own[l].end(), pyramid);
  }
  std::vector<std::vector<DetCand>> cand((size_t)L.n);
  bool overflow = false;
  for (int l = 0; l < DET_MAX_LAYERS; ++l) layer_counts[l] = 0;
  for (int l = 0; l < L.n; ++l) {
    std::vector<int64_t> S;
    det_layer_candidates_serial(view[l].pix, L.w[l], L.h[l], view[l].stride, threshold, S, cand[l]);
    if (score)
      for (int64_t s : S) *score++ = s == DET_OUTSIDE ? 0 : s;
    layer_counts[l] = (int32_t)cand[l].size();
    overflow = overflow || (int64_t)cand[l].size() > cand_capacity;
  }
  DetResult R = {0, 0, 0, 0};
  if (overflow) {   // the cross-layer test is not run; with one layer every candidate survives, and their number is known
    R.flags = DET_OVERFLOW;
    if (L.n == 1) R.n_candidates = layer_counts[0];
    return R;
  }
  std::vector<DetCand> pool;
  std::vector<DetScaleExtra> poolx;
  for (int l = 0; l < L.n; ++l)
    for (const DetCand& c : cand[l]) {
      const DetSurvivor r = det_cross(c, l, l + 1 < L.n, view[l ? l - 1 : 0], view[l], view[l + 1], kp_size);
      if (r.alive) pool.push_back(r.c), poolx.push_back(r.e);
    }
  R.n_candidates = (int32_t)pool.size();
  if ((int64_t)pool.size() > cand_capacity) {
    R.flags = DET_OVERFLOW;
    return R;
  }
  const DetScaledOrder order{pool.data(), poolx.data(), sel, selx, det_scaled_reach(min_dist)};
  R.n_keypoints = det_select_serial(order, (int)pool.size(), max_keypoints, R.flags);
  return R;
}

#if defined(__HIPCC__)
struct DetScaleJob {   // one job as the device sees it; its layers are the records img0 .. img0 + n_layers - 1 of the image table
  int64_t pix[DET_MAX_LAYERS];   // where each layer's bytes start in the pixel pool (rows packed)
  int32_t w[DET_MAX_LAYERS], h[DET_MAX_LAYERS];
  int32_t img0, n_layers;
  int32_t pool0, cap;     // its pooled survivors: records pool0 .. pool0 + cap - 1
  int32_t sel0, max_kp;   // its selected keypoints: records sel0 .. sel0 + max_kp - 1
  int32_t min_dist;
  float kp_size;
};
struct DetLayerRef { int32_t job, layer; };   // of one record of the image table
struct DetScaleParams {
  uint8_t* pix;                // the pixel pool: the images, and behind them the layers 1.. (written by detect_pyramid_kernel)
  const DetImage* images;      // per (job, layer): what detect_score_kernel reads
  const DetLayerRef* refs;     // per (job, layer)
  const DetScaleJob* jobs;
  const DetTile* pyr_tiles;    // the tiles of layer 0 of the jobs with more than one layer; .job is the job
  const int32_t* count;        // per (job, layer): candidates found by detect_score_kernel
  const DetCand* cand;
  int32_t* pool_count;         // [n_jobs] survivors found, zero on entry
  DetCand* pool;
  DetScaleExtra* poolx;
  DetCand* sel;
  DetScaleExtra* selx;
  DetResult* res;              // [n_jobs]
  int32_t* layer_count;        // [n_jobs][DET_MAX_LAYERS]
};

constexpr int DET_PYR_THREADS = 256;
static_assert(DET_TILE_X * DET_TILE_Y == 4 * DET_PYR_THREADS, "four pixels of layer 0 per lane, then at most one of a coarser layer");

__global__ void __launch_bounds__(DET_PYR_THREADS) detect_pyramid_kernel(const DetScaleParams P) {
  __shared__ uint8_t lds[DET_TILE_X * DET_TILE_Y * 2];   // layer l of the tile (1024 >> 2l bytes) at offset 2048 - (2048 >> l)
  const int tid = threadIdx.x;
  const DetTile tile = P.pyr_tiles[blockIdx.x];
  const DetScaleJob J = P.jobs[tile.job];
  {
    const uint8_t* src = P.pix + J.pix[0];
    const int ty = tid / (DET_TILE_X / 4), tx = (tid - ty * (DET_TILE_X / 4)) * 4;
    const int y = tile.y0 + ty;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = tile.x0 + tx + k;
      lds[ty * DET_TILE_X + tx + k] = (x < J.w[0] && y < J.h[0]) ? src[(int64_t)y * J.w[0] + x] : (uint8_t)0;   // a pixel beyond the image feeds no pixel of a layer
    }
  }
  __syncthreads();
#pragma unroll
  for (int l = 1; l < DET_MAX_LAYERS; ++l) {
    if (l >= J.n_layers) break;   // the same for the whole workgroup
    const int fw = DET_TILE_X >> (l - 1), lw = DET_TILE_X >> l, lh = DET_TILE_Y >> l;
    const uint8_t* from = lds + (2048 - (2048 >> (l - 1)));
    uint8_t* to = lds + (2048 - (2048 >> l));
    if (tid < lw * lh) {
      const int ty = tid / lw, tx = tid - ty * lw;
      const uint8_t* r = from + 2 * ty * fw + 2 * tx;
      const uint8_t v = det_half(r[0], r[1], r[fw], r[fw + 1]);
      to[ty * lw + tx] = v;
      const int x = (tile.x0 >> l) + tx, y = (tile.y0 >> l) + ty;   // x < w_l puts 2x + 1 < w_{l-1}: what v came from lies in the image
      if (x < J.w[l] && y < J.h[l]) P.pix[J.pix[l] + (int64_t)y * J.w[l] + x] = v;
    }
    __syncthreads();
  }
}

constexpr int DET_CROSS_THREADS = 256;

__global__ void __launch_bounds__(DET_CROSS_THREADS) detect_cross_kernel(const DetScaleParams P) {
  const int tid = threadIdx.x, img = blockIdx.x;
  const DetLayerRef ref = P.refs[img];
  const DetScaleJob& J = P.jobs[ref.job];   // read where it lies: the layer indexes it
  const int l = ref.layer, n_layers = J.n_layers;
  bool overflow = false;   // any layer: no partial result, nothing is pooled
#pragma unroll
  for (int k = 0; k < DET_MAX_LAYERS; ++k)
    if (k < n_layers) overflow = overflow || P.count[J.img0 + k] > P.images[J.img0 + k].cap;
  if (overflow) return;
  const bool has_coarse = l + 1 < n_layers;
  const int lf = l >= 1 ? l - 1 : 0, lc = has_coarse ? l + 1 : l;   // layers that exist, read or not
  const DetLayerView fine{P.pix + J.pix[lf], J.w[lf], J.w[lf], J.h[lf]}, own{P.pix + J.pix[l], J.w[l], J.w[l], J.h[l]};
  const DetLayerView coarse{P.pix + J.pix[lc], J.w[lc], J.w[lc], J.h[lc]};
  const float kp_size = J.kp_size;
  const int cap = J.cap, pool0 = J.pool0;
  const int n = P.count[img];   // <= the layer's capacity here
  const DetCand* cand = P.cand + P.images[img].cand0;
  for (int i = tid; i < n; i += DET_CROSS_THREADS) {
    const DetSurvivor r = det_cross(cand[i], l, has_coarse, fine, own, coarse, kp_size);
    if (!r.alive) continue;
    const int slot = atomicAdd(P.pool_count + ref.job, 1);   // the true count, past the capacity too
    if (slot < cap) P.pool[pool0 + slot] = r.c, P.poolx[pool0 + slot] = r.e;
  }
}

__global__ void __launch_bounds__(DET_SEL_THREADS) detect_select_scaled_kernel(const DetScaleParams P) {
  const int tid = threadIdx.x, job = blockIdx.x;
  const DetScaleJob J = P.jobs[job];
  bool overflow = false;
#pragma unroll
  for (int l = 0; l < DET_MAX_LAYERS; ++l)
    if (l < J.n_layers) overflow = overflow || P.count[J.img0 + l] > P.images[J.img0 + l].cap;
  if (tid < DET_MAX_LAYERS) P.layer_count[job * DET_MAX_LAYERS + tid] = tid < J.n_layers ? P.count[J.img0 + tid] : 0;
  // after a layer overflow nothing was pooled; with one layer every candidate survives, and their number is known
  const int n = overflow ? (J.n_layers == 1 ? P.count[J.img0] : 0) : P.pool_count[job];
  DetResult R = {0, n, 0, 0};
  if (overflow || n > J.cap) {   // the same for every lane
    R.flags = DET_OVERFLOW;
  } else {
    const DetScaledOrder order{P.pool + J.pool0, P.poolx + J.pool0, P.sel + J.sel0, P.selx + J.sel0, det_scaled_reach(J.min_dist)};
    R.n_keypoints = det_select_rounds(order, n, J.max_kp, R.flags);
  }
  if (tid == 0) P.res[job] = R;
}
#endif  // __HIPCC__

}  // namespace fe
