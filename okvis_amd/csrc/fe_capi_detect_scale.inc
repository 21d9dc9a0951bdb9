// Part of fe_capi.hip (one translation unit).  Keypoint detection over a scale space: the pyramid behind the images in the pixel
// pool, the one-layer score kernel on every (job, layer), the cross-layer test, one selection per job; alone
// (okvis_fe_detect_keypoints_scaled) and with the describe kernels behind it (okvis_fe_detect_scaled_and_describe).
// DetectScaleStage is one call's work in steps, like DetectStage.
namespace {

struct DetectScaleStage {
  int32_t n_jobs = 0;
  okvis_fe_detect_scale_job* jobs = nullptr;
  size_t n_pix = 0, n_pyr = 0, n_imgs = 0, n_tiles = 0, n_pyr_tiles = 0, n_cand = 0, n_pool = 0, n_sel = 0, n_score = 0;
  bool want_pyr = false;
  Staged<uint8_t> s_pix;
  Staged<fe::DetImage> s_images;
  Staged<fe::DetTile> s_tiles;
  Staged<int32_t> s_count;
  Staged<fe::DetLayerRef> s_refs;
  Staged<fe::DetScaleJob> s_jobs;
  Staged<fe::DetTile> s_pyr_tiles;
  Staged<int32_t> s_pool_count;
  Staged<fe::DetCand> s_cand;
  Staged<fe::DetCand> s_pool;
  Staged<fe::DetScaleExtra> s_poolx;
  Staged<uint8_t> s_pyr;
  Staged<fe::DetResult> s_res;
  Staged<fe::DetCand> s_sel;
  Staged<fe::DetScaleExtra> s_selx;
  Staged<int32_t> s_layer_count;
  Staged<int64_t> s_score;

  static size_t tiles_of(int w, int h) { return (size_t)((w + fe::DET_TILE_X - 1) / fe::DET_TILE_X) * (size_t)((h + fe::DET_TILE_Y - 1) / fe::DET_TILE_Y); }
  // a layer's list never needs more room than the layer can have candidates; it overflows exactly when it passes cand_capacity
  static int32_t layer_cap(int32_t cand_capacity, int w, int h) { return std::min(cand_capacity, fe::det_layer_bound(w, h)); }

  // every check before anything is enqueued or written
  int check(int32_t n, okvis_fe_detect_scale_job* table) {
    n_jobs = n, jobs = table;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_detect_scale_job& J = jobs[j];
      if (!J.image || !J.kp) return OKVIS_BA_ERR_ARG;
      if (!image_ok(J.image, J.width, J.height, J.pitch)) return OKVIS_BA_ERR_ARG;
      if (J.threshold < 1 || J.min_dist < 0 || J.max_keypoints < 1 || J.max_keypoints > fe::DET_MAX_KEYPOINTS || J.cand_capacity < 1 ||
          J.cand_capacity > fe::DET_MAX_CANDIDATES || J.octaves < 0 || J.octaves > fe::DET_MAX_OCTAVES)
        return OKVIS_BA_ERR_ARG;
      const fe::DetLayers L = fe::det_layers(J.width, J.height, J.octaves);
      n_pix += pool_bytes(J.width, J.height);
      for (int l = 0; l < L.n; ++l) {
        if (l) n_pyr += pool_bytes(L.w[l], L.h[l]);
        n_tiles += tiles_of(L.w[l], L.h[l]);
        n_cand += (size_t)layer_cap(J.cand_capacity, L.w[l], L.h[l]);
        if (J.score) n_score += (size_t)L.w[l] * L.h[l];
      }
      n_imgs += (size_t)L.n;
      if (L.n > 1) n_pyr_tiles += tiles_of(J.width, J.height);
      n_pool += (size_t)J.cand_capacity, n_sel += (size_t)J.max_keypoints;
      want_pyr = want_pyr || (J.pyramid && L.n > 1);
    }
    if (n_tiles > (size_t)INT32_MAX || n_cand > (size_t)INT32_MAX || n_pool > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
    return OKVIS_BA_OK;
  }
  // the pixels first and on their own, as in DetectStage
  void plan_in(Stage& st) {
    s_pix = st.in<uint8_t>(n_pix);
    s_images = st.in<fe::DetImage>(n_imgs);
    s_tiles = st.in<fe::DetTile>(n_tiles);
    s_count = st.in<int32_t>(n_imgs);
    s_refs = st.in<fe::DetLayerRef>(n_imgs);
    s_jobs = st.in<fe::DetScaleJob>((size_t)n_jobs);
    s_pyr_tiles = st.in<fe::DetTile>(n_pyr_tiles, n_pyr_tiles > 0);
    s_pool_count = st.in<int32_t>((size_t)n_jobs);
  }
  void plan_scratch(Stage& st) {
    s_cand = st.scratch<fe::DetCand>(n_cand);
    s_pool = st.scratch<fe::DetCand>(n_pool);
    s_poolx = st.scratch<fe::DetScaleExtra>(n_pool);
    if (!want_pyr) s_pyr = st.scratch<uint8_t>(n_pyr, n_pyr > 0);
  }
  void plan_out(Stage& st) {
    s_res = st.out<fe::DetResult>((size_t)n_jobs);
    s_sel = st.out<fe::DetCand>(n_sel);
    s_selx = st.out<fe::DetScaleExtra>(n_sel);
    s_layer_count = st.out<int32_t>((size_t)n_jobs * fe::DET_MAX_LAYERS);
    s_score = st.out<int64_t>(n_score, n_score > 0);
    if (want_pyr) s_pyr = st.out<uint8_t>(n_pyr);   // a referee asked for the layers: they come back with the outputs
  }
  void fill(const Stage& st) const {
    uint8_t* pix = st.host(s_pix);
    fe::DetImage* images = st.host(s_images);
    fe::DetTile* tiles = st.host(s_tiles);
    fe::DetTile* pyr_tiles = st.host(s_pyr_tiles);
    fe::DetLayerRef* refs = st.host(s_refs);
    fe::DetScaleJob* dev_jobs = st.host(s_jobs);
    std::memset(st.host(s_count), 0, s_count.bytes());
    std::memset(st.host(s_pool_count), 0, s_pool_count.bytes());
    size_t at_pix = 0, at_pyr = 0, at_img = 0, at_tile = 0, at_pyr_tile = 0, at_cand = 0, at_pool = 0, at_sel = 0, at_score = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_detect_scale_job& J = jobs[j];
      const fe::DetLayers L = fe::det_layers(J.width, J.height, J.octaves);
      fe::DetScaleJob& D = dev_jobs[j];
      std::memset(&D, 0, sizeof(D));
      D.img0 = (int32_t)at_img, D.n_layers = L.n, D.pool0 = (int32_t)at_pool, D.cap = J.cand_capacity, D.sel0 = (int32_t)at_sel;
      D.max_kp = J.max_keypoints, D.min_dist = J.min_dist, D.kp_size = J.kp_size;
      pool_image(pix + at_pix, J.image, J.width, J.height, J.pitch);
      for (int l = 0; l < L.n; ++l) {
        // the layers 1.. lie in an array of their own behind the images: one pool for the kernels, addressed from its start
        D.pix[l] = l ? (int64_t)(s_pyr.off - s_pix.off + at_pyr) : (int64_t)at_pix;
        D.w[l] = L.w[l], D.h[l] = L.h[l];
        fe::DetImage& I = images[at_img];
        I.threshold = J.threshold, I.pix = D.pix[l], I.score = J.score ? (int64_t)at_score : -1;
        I.w = L.w[l], I.h = L.h[l], I.cand0 = (int32_t)at_cand, I.cap = layer_cap(J.cand_capacity, L.w[l], L.h[l]);
        I.sel0 = 0, I.max_kp = 0, I.min_dist = 0, I.reserved = 0;   // the selection is the job's, not the layer's
        refs[at_img] = fe::DetLayerRef{j, l};
        for (int y0 = 0; y0 < L.h[l]; y0 += fe::DET_TILE_Y)
          for (int x0 = 0; x0 < L.w[l]; x0 += fe::DET_TILE_X) tiles[at_tile++] = fe::DetTile{(int32_t)at_img, x0, y0, 0};
        if (l) at_pyr += pool_bytes(L.w[l], L.h[l]);
        at_cand += (size_t)I.cap;
        if (J.score) at_score += (size_t)L.w[l] * L.h[l];
        ++at_img;
      }
      if (L.n > 1)
        for (int y0 = 0; y0 < J.height; y0 += fe::DET_TILE_Y)
          for (int x0 = 0; x0 < J.width; x0 += fe::DET_TILE_X) pyr_tiles[at_pyr_tile++] = fe::DetTile{j, x0, y0, 0};
      at_pix += pool_bytes(J.width, J.height);
      at_pool += (size_t)J.cand_capacity, at_sel += (size_t)J.max_keypoints;
    }
  }
  int launch(const Stage& st) const {
    fe::DetScaleParams P;
    P.pix = st.dev(s_pix), P.images = st.dev(s_images), P.refs = st.dev(s_refs), P.jobs = st.dev(s_jobs), P.pyr_tiles = st.dev(s_pyr_tiles);
    P.count = st.dev(s_count), P.cand = st.dev(s_cand), P.pool_count = st.dev(s_pool_count), P.pool = st.dev(s_pool), P.poolx = st.dev(s_poolx);
    P.sel = st.dev(s_sel), P.selx = st.dev(s_selx), P.res = st.dev(s_res), P.layer_count = st.dev(s_layer_count);
    fe::DetParams Q;   // the one-layer score kernel on the (job, layer) table; it reads no selection field
    Q.pix = P.pix, Q.images = P.images, Q.tiles = st.dev(s_tiles), Q.count = st.dev(s_count), Q.cand = st.dev(s_cand);
    Q.sel = nullptr, Q.res = nullptr, Q.score = st.dev(s_score);
    if (n_pyr_tiles) {
      hipLaunchKernelGGL(fe::detect_pyramid_kernel, dim3((unsigned)n_pyr_tiles), dim3(fe::DET_PYR_THREADS), 0, st.c->stream, P);
      FE_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(fe::detect_score_kernel, dim3((unsigned)n_tiles), dim3(fe::DET_THREADS), 0, st.c->stream, Q);
    FE_TRY(hipGetLastError());
    hipLaunchKernelGGL(fe::detect_cross_kernel, dim3((unsigned)n_imgs), dim3(fe::DET_CROSS_THREADS), 0, st.c->stream, P);
    FE_TRY(hipGetLastError());
    hipLaunchKernelGGL(fe::detect_select_scaled_kernel, dim3((unsigned)n_jobs), dim3(fe::DET_SEL_THREADS), 0, st.c->stream, P);
    FE_TRY(hipGetLastError());
    return OKVIS_BA_OK;
  }
  void unpack(const Stage& st) const {
    const fe::DetResult* res = st.host(s_res);
    const fe::DetScaleJob* dev_jobs = st.host(s_jobs);
    const fe::DetImage* images = st.host(s_images);
    for (int j = 0; j < n_jobs; ++j) {
      okvis_fe_detect_scale_job& J = jobs[j];
      const fe::DetResult& R = res[j];
      const fe::DetScaleJob& D = dev_jobs[j];
      J.n_keypoints = R.n_keypoints, J.n_candidates = R.n_candidates, J.flags = R.flags, J.n_layers = D.n_layers;
      std::memcpy(J.n_layer_candidates, st.host(s_layer_count) + (size_t)j * fe::DET_MAX_LAYERS, sizeof(J.n_layer_candidates));
      const fe::DetCand* sel = st.host(s_sel) + D.sel0;
      const fe::DetScaleExtra* selx = st.host(s_selx) + D.sel0;
      for (int i = 0; i < R.n_keypoints; ++i) {
        J.kp[3 * (size_t)i] = sel[i].fx, J.kp[3 * (size_t)i + 1] = sel[i].fy, J.kp[3 * (size_t)i + 2] = selx[i].size;
        if (J.response) J.response[i] = (double)sel[i].s;
        if (J.pixel) J.pixel[2 * (size_t)i] = sel[i].x, J.pixel[2 * (size_t)i + 1] = sel[i].y;
        if (J.layer) J.layer[i] = selx[i].layer;
        if (J.scale) J.scale[i] = selx[i].scale;
      }
      size_t at_score = 0, at_pyr = 0;
      for (int l = 0; l < D.n_layers; ++l) {
        const size_t px = (size_t)D.w[l] * D.h[l];
        if (J.score) std::memcpy(J.score + at_score, st.host(s_score) + images[D.img0 + l].score, sizeof(int64_t) * px);
        if (J.pyramid && l) std::memcpy(J.pyramid + at_pyr, st.host(s_pix) + D.pix[l], px), at_pyr += px;
        at_score += px;
      }
    }
  }
};

// the describe stage takes its images, row counts and selection ranges from one-layer detect records: the scaled jobs as such
struct ScaledChain {
  std::vector<okvis_fe_detect_job> det;
  std::vector<fe::DetImage> images;
  explicit ScaledChain(int32_t n, const okvis_fe_detect_scale_job* jobs) : det((size_t)std::max(n, 0)) {
    for (int j = 0; j < n; ++j) {
      okvis_fe_detect_job& d = det[j];
      std::memset(&d, 0, sizeof(d));
      d.image = jobs[j].image, d.width = jobs[j].width, d.height = jobs[j].height, d.pitch = jobs[j].pitch, d.max_keypoints = jobs[j].max_keypoints;
    }
  }
  void fill(const Stage& st, const DetectScaleStage& D) {
    images.resize(det.size());
    const fe::DetScaleJob* dev_jobs = st.host(D.s_jobs);
    for (size_t j = 0; j < det.size(); ++j) {
      std::memset(&images[j], 0, sizeof(fe::DetImage));
      images[j].pix = dev_jobs[j].pix[0], images[j].w = dev_jobs[j].w[0], images[j].h = dev_jobs[j].h[0], images[j].sel0 = dev_jobs[j].sel0;
    }
  }
};

}  // namespace

extern "C" {

int okvis_fe_detect_keypoints_scaled(okvis_fe_context* c, int32_t n_jobs, okvis_fe_detect_scale_job* jobs) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs)) return OKVIS_BA_ERR_ARG;
  DetectScaleStage D;
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

int okvis_fe_detect_scaled_and_describe(okvis_fe_context* c, int32_t n_jobs, okvis_fe_detect_scale_job* det, okvis_fe_describe_job* desc) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && (!det || !desc))) return OKVIS_BA_ERR_ARG;
  DetectScaleStage D;
  DescribeStage B;
  if (int rc = D.check(n_jobs, det)) return rc;
  ScaledChain chain(n_jobs, det);
  if (int rc = B.check(n_jobs, desc, chain.det.data())) return rc;
  if (n_jobs == 0) return OKVIS_BA_OK;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  // the images once; the describe kernels read the selected keypoints where detect_select_scaled_kernel leaves them
  D.plan_in(st), B.plan_in(st), D.plan_scratch(st), D.plan_out(st), B.plan_out(st);
  if (int rc = st.reserve()) return rc;
  D.fill(st);
  chain.fill(st, D);
  B.fill(st, chain.images.data());
  if (int rc = st.upload()) return rc;
  if (int rc = D.launch(st)) return rc;
  if (int rc = B.launch(st, st.dev(D.s_pix), st.dev(D.s_sel), st.dev(D.s_res))) return rc;
  if (int rc = st.download()) return rc;
  D.unpack(st);
  B.unpack(st, st.host(D.s_res));
  return OKVIS_BA_OK;
}

}  // extern "C"
