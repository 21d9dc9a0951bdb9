// Part of fe_capi.hip (one translation unit).  Keypoint description: the angle per keypoint and the 48-byte descriptor, on their own
// (okvis_fe_describe_keypoints) and behind the kernels of a detect stage on the keypoints they left in device memory
// (run_detect_describe: okvis_fe_detect_and_describe here, okvis_fe_detect_scaled_and_describe in fe_capi_detect_scale.inc).
// DescribeStage is one call's describe work in steps, like DetectStage.  Of a detect stage in front of it, it knows one
// DescribeSource per job and the device arrays of the selection.
namespace {

struct DescribeStage {
  int32_t n_jobs = 0;
  okvis_fe_describe_job* jobs = nullptr;
  const DescribeSource* src = nullptr;   // per job: its image and its rows
  std::vector<DescribeSource> own;       // ... made here from the jobs, unless a detect stage in front handed its own out
  bool chained = false;                  // images, keypoints and counts are the detect stage's
  size_t n_pix = 0, n_rows = 0, n_cams = 0;
  bool want_angle = false, want_angle64 = false;
  Staged<uint8_t> s_pix;
  Staged<fe::DscImage> s_images;
  Staged<int32_t> s_row_job;
  Staged<fe::DscCamera> s_cams;
  Staged<float> s_kp;
  Staged<int32_t> s_rot_in;
  Staged<int32_t> s_rot;
  Staged<float> s_angle;
  Staged<double> s_angle64;
  Staged<uint8_t> s_flags;
  Staged<uint8_t> s_desc;

  // every check before anything is enqueued or written; chain: the sources of a detect stage whose check has passed, or null
  int check(int32_t n, okvis_fe_describe_job* table, const DescribeSource* chain) {
    n_jobs = n, jobs = table, src = chain, chained = chain != nullptr;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_describe_job& J = jobs[j];
      if (!J.desc || !J.flags) return OKVIS_BA_ERR_ARG;
      if (!chained) {
        if (!J.kp || J.n < 0 || !image_ok(J.image, J.width, J.height, J.pitch)) return OKVIS_BA_ERR_ARG;
        own.push_back(DescribeSource{(int64_t)n_pix, J.width, J.height, 0, J.n});
        n_pix += pool_bytes(J.width, J.height);
      }
      const int rows = chained ? src[j].rows : J.n;
      if (J.rot_in) {
        for (int i = 0; i < rows; ++i)
          if (J.rot_in[i] < 0 || J.rot_in[i] >= fe::DSC_ROTS) return OKVIS_BA_ERR_ARG;
      } else {
        if (!camera_ok(J.cam)) return OKVIS_BA_ERR_ARG;
        ++n_cams;
      }
      n_rows += (size_t)rows;
      want_angle = want_angle || (J.angle && !J.rot_in), want_angle64 = want_angle64 || (J.angle64 && !J.rot_in);
    }
    if (n_rows > (size_t)INT32_MAX / fe::DSC_BYTES) return OKVIS_BA_ERR_ARG;
    if (!chained) src = own.data();
    return OKVIS_BA_OK;
  }
  void plan_in(Stage& st) {
    if (!chained) s_pix = st.in<uint8_t>(n_pix);
    s_images = st.in<fe::DscImage>((size_t)n_jobs);
    s_row_job = st.in<int32_t>(n_rows);
    s_cams = st.in<fe::DscCamera>(n_cams, n_cams > 0);
    s_kp = st.in<float>(3 * n_rows, !chained);
    s_rot_in = st.in<int32_t>(n_rows, n_cams < (size_t)n_jobs);
  }
  void plan_out(Stage& st) {
    s_rot = st.out<int32_t>(n_rows);
    s_angle = st.out<float>(n_rows, want_angle);
    s_angle64 = st.out<double>(n_rows, want_angle64);
    s_flags = st.out<uint8_t>(n_rows);
    s_desc = st.out<uint8_t>((size_t)fe::DSC_BYTES * n_rows);
  }
  void fill(const Stage& st) const {
    fe::DscImage* images = st.host(s_images);
    int32_t* row_job = st.host(s_row_job);
    size_t at_row = 0, at_cam = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_describe_job& J = jobs[j];
      const DescribeSource& S = src[j];
      fe::DscImage& I = images[j];
      const int rows = S.rows;
      I.pix = S.pix, I.w = S.w, I.h = S.h, I.kp0 = (int32_t)at_row, I.sel0 = S.sel0, I.reserved = 0;
      I.n = chained ? -1 : J.n, I.det = chained ? j : -1;   // chained: the count is the detect result's
      if (!chained) {
        pool_image(st.host(s_pix) + S.pix, J.image, J.width, J.height, J.pitch);
        if (rows) std::memcpy(st.host(s_kp) + 3 * at_row, J.kp, sizeof(float) * 3 * (size_t)rows);
      }
      if (J.rot_in) {
        I.cam = -1;
        if (rows) std::memcpy(st.host(s_rot_in) + at_row, J.rot_in, sizeof(int32_t) * (size_t)rows);
      } else {
        I.cam = (int32_t)at_cam;
        fe::DscCamera& C = st.host(s_cams)[at_cam++];
        C.cam = to_device(J.cam);
        std::memcpy(C.dir, J.direction, sizeof(C.dir));
        if (s_rot_in.on && rows) std::memset(st.host(s_rot_in) + at_row, 0, sizeof(int32_t) * (size_t)rows);
      }
      for (int i = 0; i < rows; ++i) row_job[at_row + i] = j;
      at_row += (size_t)rows;
    }
  }
  int launch(const Stage& st, const uint8_t* pix, const fe::DetCand* sel, const fe::DetResult* det_res) const {
    if (n_rows == 0) return OKVIS_BA_OK;
    fe::DscParams P;
    P.pix = pix, P.images = st.dev(s_images), P.row_job = st.dev(s_row_job), P.kp = st.dev(s_kp), P.sel = sel, P.det_res = det_res;
    P.cams = st.dev(s_cams), P.rot_in = st.dev(s_rot_in), P.rot = st.dev(s_rot), P.angle = st.dev(s_angle), P.angle64 = st.dev(s_angle64);
    P.flags = st.dev(s_flags), P.desc = st.dev(s_desc), P.rows = (int32_t)n_rows;
    hipLaunchKernelGGL(fe::describe_angle_kernel, dim3((unsigned)((n_rows + fe::DSC_ANGLE_THREADS - 1) / fe::DSC_ANGLE_THREADS)),
                       dim3(fe::DSC_ANGLE_THREADS), 0, st.c->stream, P);
    FE_TRY(hipGetLastError());
    hipLaunchKernelGGL(fe::describe_kernel, dim3((unsigned)((n_rows + fe::DSC_WAVES - 1) / fe::DSC_WAVES)), dim3(fe::DSC_THREADS), 0,
                       st.c->stream, P);
    FE_TRY(hipGetLastError());
    return OKVIS_BA_OK;
  }
  // det_res: the detect stage's results, whose counts are the keypoints each job really has (null without a chain)
  void unpack(const Stage& st, const fe::DetResult* det_res) const {
    const fe::DscImage* images = st.host(s_images);
    for (int j = 0; j < n_jobs; ++j) {
      okvis_fe_describe_job& J = jobs[j];
      const size_t n = (size_t)(det_res ? det_res[j].n_keypoints : J.n), at = (size_t)images[j].kp0;
      int32_t n_valid = 0;
      const uint8_t* flags = st.host(s_flags) + at;
      for (size_t i = 0; i < n; ++i) n_valid += flags[i] & fe::DSC_VALID;
      J.n_valid = n_valid;
      if (n == 0) continue;
      std::memcpy(J.desc, st.host(s_desc) + (size_t)fe::DSC_BYTES * at, (size_t)fe::DSC_BYTES * n);
      std::memcpy(J.flags, flags, n);
      if (J.rot) std::memcpy(J.rot, st.host(s_rot) + at, sizeof(int32_t) * n);
      if (J.angle && !J.rot_in) std::memcpy(J.angle, st.host(s_angle) + at, sizeof(float) * n);
      if (J.angle64 && !J.rot_in) std::memcpy(J.angle64, st.host(s_angle64) + at, sizeof(double) * n);
    }
  }
};

// one call of a detect stage D with the describe stage behind it: the images staged once, the describe kernels read the selected
// keypoints where D's selection kernel leaves them
template <class D>
int run_detect_describe(okvis_fe_context* c, int32_t n_jobs, typename D::Job* det, okvis_fe_describe_job* desc) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && (!det || !desc))) return OKVIS_BA_ERR_ARG;
  D d;
  DescribeStage B;
  if (int rc = d.check(n_jobs, det)) return rc;
  if (n_jobs == 0) return OKVIS_BA_OK;
  if (int rc = B.check(n_jobs, desc, d.src.data())) return rc;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  d.plan_in(st), B.plan_in(st), d.plan_scratch(st), d.plan_out(st), B.plan_out(st);
  if (int rc = st.reserve()) return rc;
  d.fill(st);
  B.fill(st);
  if (int rc = st.upload()) return rc;
  if (int rc = d.launch(st)) return rc;
  if (int rc = B.launch(st, st.dev(d.s_pix), st.dev(d.s_sel), st.dev(d.s_res))) return rc;
  if (int rc = st.download()) return rc;
  d.unpack(st);
  B.unpack(st, st.host(d.s_res));
  return OKVIS_BA_OK;
}

}  // namespace

extern "C" {

int okvis_fe_describe_keypoints(okvis_fe_context* c, int32_t n_jobs, okvis_fe_describe_job* jobs) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs)) return OKVIS_BA_ERR_ARG;
  DescribeStage B;
  if (int rc = B.check(n_jobs, jobs, nullptr)) return rc;
  if (B.n_rows == 0) {   // no keypoint anywhere: nothing to stage
    for (int j = 0; j < n_jobs; ++j) jobs[j].n_valid = 0;
    return OKVIS_BA_OK;
  }
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  B.plan_in(st), B.plan_out(st);
  if (int rc = st.reserve()) return rc;
  B.fill(st);
  if (int rc = st.upload()) return rc;
  if (int rc = B.launch(st, st.dev(B.s_pix), nullptr, nullptr)) return rc;
  if (int rc = st.download()) return rc;
  B.unpack(st, nullptr);
  return OKVIS_BA_OK;
}

int okvis_fe_detect_and_describe(okvis_fe_context* c, int32_t n_jobs, okvis_fe_detect_job* det, okvis_fe_describe_job* desc) {
  return run_detect_describe<DetectStage>(c, n_jobs, det, desc);
}

int okvis_fe_describe_tables(const int32_t** cs, const int32_t** base, const uint8_t** ring, const int32_t** half, const uint8_t** pairs,
                             int32_t* n_pairs) {
  if (!cs || !base || !ring || !half || !pairs || !n_pairs) return OKVIS_BA_ERR_ARG;
  *cs = &fe::dsc_host::dsc_cs[0][0], *base = &fe::dsc_host::dsc_base[0][0], *ring = fe::dsc_host::dsc_ring, *half = fe::dsc_host::dsc_half;
  *pairs = &fe::dsc_host::dsc_pairs[0][0], *n_pairs = fe::DSC_PAIRS;
  return OKVIS_BA_OK;
}

}  // extern "C"
