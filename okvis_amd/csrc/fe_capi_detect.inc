// Part of fe_capi.hip (one translation unit).  Keypoint detection: Harris scores and candidates per tile, selection per image.
// DetectStage is one call's detect work in steps, so that okvis_fe_detect_and_describe (fe_capi_describe.inc) runs the same checks,
// the same staging and the same two launches with the describe arrays planned around them.
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

struct DetectStage {
  int32_t n_jobs = 0;
  okvis_fe_detect_job* jobs = nullptr;
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
  int check(int32_t n, okvis_fe_detect_job* table) {
    n_jobs = n, jobs = table;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_detect_job& J = jobs[j];
      if (!J.image || !J.kp) return OKVIS_BA_ERR_ARG;
      if (!image_ok(J.image, J.width, J.height, J.pitch)) return OKVIS_BA_ERR_ARG;
      if (J.threshold < 1 || J.min_dist < 0 || J.max_keypoints < 1 || J.max_keypoints > fe::DET_MAX_KEYPOINTS || J.cand_capacity < 1 ||
          J.cand_capacity > fe::DET_MAX_CANDIDATES)
        return OKVIS_BA_ERR_ARG;
      n_pix += pool_bytes(J.width, J.height);
      n_tiles += (size_t)((J.width + fe::DET_TILE_X - 1) / fe::DET_TILE_X) * (size_t)((J.height + fe::DET_TILE_Y - 1) / fe::DET_TILE_Y);
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
    uint8_t* pix = st.host(s_pix);
    fe::DetImage* images = st.host(s_images);
    fe::DetTile* tiles = st.host(s_tiles);
    std::memset(st.host(s_count), 0, s_count.bytes());
    size_t at_pix = 0, at_tile = 0, at_cand = 0, at_sel = 0, at_score = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_detect_job& J = jobs[j];
      fe::DetImage& I = images[j];
      I.threshold = J.threshold, I.pix = (int64_t)at_pix, I.score = J.score ? (int64_t)at_score : -1;
      I.w = J.width, I.h = J.height, I.cand0 = (int32_t)at_cand, I.cap = J.cand_capacity, I.sel0 = (int32_t)at_sel, I.max_kp = J.max_keypoints;
      I.min_dist = J.min_dist, I.reserved = 0;
      pool_image(pix + at_pix, J.image, J.width, J.height, J.pitch);
      for (int y0 = 0; y0 < J.height; y0 += fe::DET_TILE_Y)
        for (int x0 = 0; x0 < J.width; x0 += fe::DET_TILE_X) tiles[at_tile++] = fe::DetTile{j, x0, y0, 0};
      at_pix += pool_bytes(J.width, J.height);
      at_cand += (size_t)J.cand_capacity, at_sel += (size_t)J.max_keypoints;
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
      okvis_fe_detect_job& J = jobs[j];
      const fe::DetResult& R = res[j];
      J.n_keypoints = R.n_keypoints, J.n_candidates = R.n_candidates, J.flags = R.flags;
      const fe::DetCand* sel = st.host(s_sel) + images[j].sel0;
      for (int i = 0; i < R.n_keypoints; ++i) {
        J.kp[3 * (size_t)i] = sel[i].fx, J.kp[3 * (size_t)i + 1] = sel[i].fy, J.kp[3 * (size_t)i + 2] = J.kp_size;
        if (J.response) J.response[i] = (double)sel[i].s;
        if (J.pixel) J.pixel[2 * (size_t)i] = sel[i].x, J.pixel[2 * (size_t)i + 1] = sel[i].y;
      }
      if (J.score) std::memcpy(J.score, st.host(s_score) + images[j].score, sizeof(int64_t) * (size_t)J.width * J.height);
    }
  }
};

}  // namespace

extern "C" {

int okvis_fe_detect_keypoints(okvis_fe_context* c, int32_t n_jobs, okvis_fe_detect_job* jobs) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs)) return OKVIS_BA_ERR_ARG;
  DetectStage D;
  if (int rc = D.check(n_jobs, jobs)) return rc;
  if (n_jobs == 0) return OKVIS_BA_OK;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  D.plan_in(st), D.plan_scratch(st), D.plan_out(st);
  if (int rc = st.reserve()) return rc;
  D.fill(st);
  if (int rc = st.upload()) return rc;
  if (int rc = D.launch(st)) return rc;
  if (int rc = st.download()) return rc;
  D.unpack(st);
  return OKVIS_BA_OK;
}

}  // extern "C"
