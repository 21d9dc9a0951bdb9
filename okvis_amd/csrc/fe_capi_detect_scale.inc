// Part of fe_capi.hip (one translation unit).  Keypoint detection over a scale space: the pyramid behind the images in the pixel
// pool, the one-layer score kernel on every (job, layer), the cross-layer test, one selection per job; alone
// (okvis_fe_detect_keypoints_scaled) and with the describe kernels behind it (okvis_fe_detect_scaled_and_describe).
// DetectScaleStage is one call's work in steps, like DetectStage, and is driven by the same run_detect / run_detect_describe.
namespace {

struct DetectScaleStage {
  using Job = okvis_fe_detect_scale_job;
  int32_t n_jobs = 0;
  Job* jobs = nullptr;
  std::vector<DescribeSource> src;
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

  // a layer's list never needs more room than the layer can have candidates; it overflows exactly when it passes cand_capacity
  static int32_t layer_cap(int32_t cand_capacity, int w, int h) { return std::min(cand_capacity, fe::det_layer_bound(w, h)); }

  // every check before anything is enqueued or written
  int check(int32_t n, Job* table) {
    n_jobs = n, jobs = table;
    for (int j = 0; j < n_jobs; ++j) {
      const Job& J = jobs[j];
      if (!detect_job_ok(J) || J.octaves < 0 || J.octaves > fe::DET_MAX_OCTAVES) return OKVIS_BA_ERR_ARG;
      const fe::DetLayers L = fe::det_layers(J.width, J.height, J.octaves);
      src.push_back(DescribeSource{(int64_t)n_pix, J.width, J.height, (int32_t)n_sel, J.max_keypoints});
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
    fe::DetImage* images = st.host(s_images);
    fe::DetTile* tile = st.host(s_tiles);
    fe::DetTile* pyr_tile = st.host(s_pyr_tiles);
    fe::DetLayerRef* refs = st.host(s_refs);
    fe::DetScaleJob* dev_jobs = st.host(s_jobs);
    std::memset(st.host(s_count), 0, s_count.bytes());
    std::memset(st.host(s_pool_count), 0, s_pool_count.bytes());
    size_t at_pyr = 0, at_img = 0, at_cand = 0, at_pool = 0, at_score = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const Job& J = jobs[j];
      const DescribeSource& S = src[j];
      const fe::DetLayers L = fe::det_layers(J.width, J.height, J.octaves);
      fe::DetScaleJob& D = dev_jobs[j];
      std::memset(&D, 0, sizeof(D));
      D.img0 = (int32_t)at_img, D.n_layers = L.n, D.pool0 = (int32_t)at_pool, D.cap = J.cand_capacity, D.sel0 = S.sel0;
      D.max_kp = S.rows, D.min_dist = J.min_dist, D.kp_size = J.kp_size;
      pool_image(st.host(s_pix) + S.pix, J.image, J.width, J.height, J.pitch);
      for (int l = 0; l < L.n; ++l) {
        // the layers 1.. lie in an array of their own behind the images: one pool for the kernels, addressed from its start
        D.pix[l] = l ? (int64_t)(s_pyr.off - s_pix.off + at_pyr) : S.pix;
        D.w[l] = L.w[l], D.h[l] = L.h[l];
        fe::DetImage& I = images[at_img];
        I.threshold = J.threshold, I.pix = D.pix[l], I.score = J.score ? (int64_t)at_score : -1;
        I.w = L.w[l], I.h = L.h[l], I.cand0 = (int32_t)at_cand, I.cap = layer_cap(J.cand_capacity, L.w[l], L.h[l]);
        I.sel0 = 0, I.max_kp = 0, I.min_dist = 0, I.reserved = 0;   // the selection is the job's, not the layer's
        refs[at_img] = fe::DetLayerRef{j, l};
        tile = emit_tiles(tile, (int32_t)at_img, L.w[l], L.h[l]);
        if (l) at_pyr += pool_bytes(L.w[l], L.h[l]);
        at_cand += (size_t)I.cap;
        if (J.score) at_score += (size_t)L.w[l] * L.h[l];
        ++at_img;
      }
      if (L.n > 1) pyr_tile = emit_tiles(pyr_tile, j, J.width, J.height);
      at_pool += (size_t)J.cand_capacity;
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
      Job& J = jobs[j];
      const fe::DetResult& R = res[j];
      const fe::DetScaleJob& D = dev_jobs[j];
      J.n_keypoints = R.n_keypoints, J.n_candidates = R.n_candidates, J.flags = R.flags, J.n_layers = D.n_layers;
      std::memcpy(J.n_layer_candidates, st.host(s_layer_count) + (size_t)j * fe::DET_MAX_LAYERS, sizeof(J.n_layer_candidates));
      const fe::DetScaleExtra* selx = st.host(s_selx) + D.sel0;
      scatter_keypoints(J, st.host(s_sel) + D.sel0, R.n_keypoints, [&](int i) { return selx[i].size; });
      for (int i = 0; i < R.n_keypoints; ++i) {
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

}  // namespace

extern "C" {

int okvis_fe_detect_keypoints_scaled(okvis_fe_context* c, int32_t n_jobs, okvis_fe_detect_scale_job* jobs) {
  return run_detect<DetectScaleStage>(c, n_jobs, jobs);
}

int okvis_fe_detect_scaled_and_describe(okvis_fe_context* c, int32_t n_jobs, okvis_fe_detect_scale_job* det, okvis_fe_describe_job* desc) {
  return run_detect_describe<DetectScaleStage>(c, n_jobs, det, desc);
}

}  // extern "C"
