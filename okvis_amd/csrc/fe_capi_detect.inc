// Part of fe_capi.hip (one translation unit).  Keypoint detection: Harris scores and candidates per tile, selection per image.
// DetectStage is one call's detect work in steps; run_detect drives a detect stage (this one, or DetectScaleStage of
// fe_capi_detect_scale.inc) alone, run_detect_describe (fe_capi_describe.inc) with the describe arrays planned around it.  What
// both detect stages need is here: the pixel pool, the check of the job fields they share, the tile table, the keypoint scatter
// and the record a describe stage behind them reads.
namespace {

// the pixel pool shared by the detect and the describe entries: rows packed without their pitch, every image 16-byte aligned
size_t pool_bytes(int width, int height) { return ((size_t)width * height + 15) & ~(size_t)15; }
bool image_ok(const uint8_t* image, int width, int height, int pitch) {
  return image && width >= fe::DET_MIN_DIM && width <= fe::DET_MAX_DIM && height >= fe::DET_MIN_DIM && height <= fe::DET_MAX_DIM && pitch >= width;
}
void pool_image(uint8_t* dst, const uint8_t* image, int width, int height, int pitch) {
  if (pitch == width)
    std::memcpy(dst, image, (size_t)width * height);
  else
    for (int y = 0; y < height; ++y) std::memcpy(dst + (size_t)y * width, image + (size_t)y * pitch, (size_t)width);
}

// the fields okvis_fe_detect_job and okvis_fe_detect_scale_job begin with, and kp
template <class Job>
bool detect_job_ok(const Job& J) {
  return J.kp && image_ok(J.image, J.width, J.height, J.pitch) && J.threshold >= 1 && J.min_dist >= 0 && J.max_keypoints >= 1 &&
         J.max_keypoints <= fe::DET_MAX_KEYPOINTS && J.cand_capacity >= 1 && J.cand_capacity <= fe::DET_MAX_CANDIDATES;
}

// the score kernel's tiles of a w x h image, and their records for image `job` of the image table
size_t tiles_of(int w, int h) { return (size_t)((w + fe::DET_TILE_X - 1) / fe::DET_TILE_X) * (size_t)((h + fe::DET_TILE_Y - 1) / fe::DET_TILE_Y); }
fe::DetTile* emit_tiles(fe::DetTile* at, int32_t job, int w, int h) {
  for (int y0 = 0; y0 < h; y0 += fe::DET_TILE_Y)
    for (int x0 = 0; x0 < w; x0 += fe::DET_TILE_X) *at++ = fe::DetTile{job, x0, y0, 0};
  return at;
}

// the n selected keypoints of a job into its kp, response and pixel; size(i): the size of keypoint i
template <class Job, class Size>
void scatter_keypoints(Job& J, const fe::DetCand* sel, int n, Size size) {
  for (int i = 0; i < n; ++i) {
    J.kp[3 * (size_t)i] = sel[i].fx, J.kp[3 * (size_t)i + 1] = sel[i].fy, J.kp[3 * (size_t)i + 2] = size(i);
    if (J.response) J.response[i] = (double)sel[i].s;
    if (J.pixel) J.pixel[2 * (size_t)i] = sel[i].x, J.pixel[2 * (size_t)i + 1] = sel[i].y;
  }
}

// What a describe stage reads of one job: its image in the pixel pool, its first record in the selection pool and the rows it
// may have.  A detect stage makes one per job in check(), where every offset is known, and fills its own records from them.
struct DescribeSource {
  int64_t pix;
  int32_t w, h, sel0, rows;
};

struct DetectStage {
  using Job = okvis_fe_detect_job;
  int32_t n_jobs = 0;
  Job* jobs = nullptr;
  std::vector<DescribeSource> src;
  size_t n_pix = 0, n_tiles = 0, n_cand = 0, n_sel = 0, n_score = 0;
  Staged<uint8_t> s_pix;
  Staged<fe::DetImage> s_images;
  Staged<fe::DetTile> s_tiles;
  Staged<int32_t> s_count;
  Staged<fe::DetCand> s_cand;
  Staged<fe::DetResult> s_res;
  Staged<fe::DetCand> s_sel;
  Staged<int64_t> s_score;

  // every check before anything is enqueued or written
  int check(int32_t n, Job* table) {
    n_jobs = n, jobs = table;
    for (int j = 0; j < n_jobs; ++j) {
      const Job& J = jobs[j];
      if (!detect_job_ok(J)) return OKVIS_BA_ERR_ARG;
      src.push_back(DescribeSource{(int64_t)n_pix, J.width, J.height, (int32_t)n_sel, J.max_keypoints});
      n_pix += pool_bytes(J.width, J.height);
      n_tiles += tiles_of(J.width, J.height);
      n_cand += (size_t)J.cand_capacity, n_sel += (size_t)J.max_keypoints;
      if (J.score) n_score += (size_t)J.width * J.height;
    }
    if (n_tiles > (size_t)INT32_MAX || n_cand > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
    return OKVIS_BA_OK;
  }
  // the pixels first and on their own: what reads the same images in the same call finds them where this left them
  void plan_in(Stage& st) {
    s_pix = st.in<uint8_t>(n_pix);
    s_images = st.in<fe::DetImage>((size_t)n_jobs);
    s_tiles = st.in<fe::DetTile>(n_tiles);
    s_count = st.in<int32_t>((size_t)n_jobs);
  }
  void plan_scratch(Stage& st) { s_cand = st.scratch<fe::DetCand>(n_cand); }
  void plan_out(Stage& st) {
    s_res = st.out<fe::DetResult>((size_t)n_jobs);
    s_sel = st.out<fe::DetCand>(n_sel);
    s_score = st.out<int64_t>(n_score, n_score > 0);
  }
  void fill(const Stage& st) const {
    fe::DetImage* images = st.host(s_images);
    fe::DetTile* tile = st.host(s_tiles);
    std::memset(st.host(s_count), 0, s_count.bytes());
    size_t at_cand = 0, at_score = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const Job& J = jobs[j];
      const DescribeSource& S = src[j];
      fe::DetImage& I = images[j];
      I.threshold = J.threshold, I.pix = S.pix, I.score = J.score ? (int64_t)at_score : -1;
      I.w = S.w, I.h = S.h, I.cand0 = (int32_t)at_cand, I.cap = J.cand_capacity, I.sel0 = S.sel0, I.max_kp = S.rows;
      I.min_dist = J.min_dist, I.reserved = 0;
      pool_image(st.host(s_pix) + S.pix, J.image, J.width, J.height, J.pitch);
      tile = emit_tiles(tile, j, S.w, S.h);
      at_cand += (size_t)J.cand_capacity;
      if (J.score) at_score += (size_t)J.width * J.height;
    }
  }
  int launch(const Stage& st) const {
    fe::DetParams P;
    P.pix = st.dev(s_pix), P.images = st.dev(s_images), P.tiles = st.dev(s_tiles), P.count = st.dev(s_count), P.cand = st.dev(s_cand);
    P.sel = st.dev(s_sel), P.res = st.dev(s_res), P.score = st.dev(s_score);
    hipLaunchKernelGGL(fe::detect_score_kernel, dim3((unsigned)n_tiles), dim3(fe::DET_THREADS), 0, st.c->stream, P);
    FE_TRY(hipGetLastError());
    hipLaunchKernelGGL(fe::detect_select_kernel, dim3((unsigned)n_jobs), dim3(fe::DET_SEL_THREADS), 0, st.c->stream, P);
    FE_TRY(hipGetLastError());
    return OKVIS_BA_OK;
  }
  void unpack(const Stage& st) const {
    const fe::DetResult* res = st.host(s_res);
    const fe::DetImage* images = st.host(s_images);
    for (int j = 0; j < n_jobs; ++j) {
      Job& J = jobs[j];
      const fe::DetResult& R = res[j];
      J.n_keypoints = R.n_keypoints, J.n_candidates = R.n_candidates, J.flags = R.flags;
      scatter_keypoints(J, st.host(s_sel) + src[j].sel0, R.n_keypoints, [&](int) { return J.kp_size; });
      if (J.score) std::memcpy(J.score, st.host(s_score) + images[j].score, sizeof(int64_t) * (size_t)J.width * J.height);
    }
  }
};

// one call of a detect stage D: every check before hipSetDevice, then one block staged, one copy in, the launches, one copy out
template <class D>
int run_detect(okvis_fe_context* c, int32_t n_jobs, typename D::Job* jobs) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs)) return OKVIS_BA_ERR_ARG;
  D d;
  if (int rc = d.check(n_jobs, jobs)) return rc;
  if (n_jobs == 0) return OKVIS_BA_OK;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  d.plan_in(st), d.plan_scratch(st), d.plan_out(st);
  if (int rc = st.reserve()) return rc;
  d.fill(st);
  if (int rc = st.upload()) return rc;
  if (int rc = d.launch(st)) return rc;
  if (int rc = st.download()) return rc;
  d.unpack(st);
  return OKVIS_BA_OK;
}

}  // namespace

extern "C" {

int okvis_fe_detect_keypoints(okvis_fe_context* c, int32_t n_jobs, okvis_fe_detect_job* jobs) { return run_detect<DetectStage>(c, n_jobs, jobs); }

}  // extern "C"
