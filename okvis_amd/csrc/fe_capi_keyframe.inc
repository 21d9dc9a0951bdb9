// Part of fe_capi.hip (one translation unit).  The keyframe decision: hulls, areas and inside counts per image, folded per job.
extern "C" {

int okvis_fe_keyframe_decision(okvis_fe_context* c, int32_t n_kp, const float* kp, const uint8_t* matched, int32_t n_images,
                               const okvis_fe_kf_image* images, int32_t n_jobs, const okvis_fe_kf_job* jobs, uint8_t* decision,
                               double* overlap, double* ratio, int32_t* n_matched, int32_t* hull_all_size, int32_t* hull_matched_size,
                               double* area_all, double* area_matched, int32_t* n_inside, uint8_t* flags, int32_t* hull_all,
                               int32_t* hull_matched) {
  if (!c || n_kp < 0 || n_images < 0 || n_jobs < 0) return OKVIS_BA_ERR_ARG;
  if ((n_jobs > 0 && !jobs) || (n_images > 0 && !images) || (n_kp > 0 && (!kp || !matched))) return OKVIS_BA_ERR_ARG;
  // every check before anything is enqueued
  size_t n_hull = 0;
  int32_t n_max = 0;
  for (int i = 0; i < n_images; ++i) {
    const okvis_fe_kf_image& I = images[i];
    if (I.kp_begin < 0 || I.kp_count < 0 || I.kp_count > fe::KF_MAX_KEYPOINTS || (int64_t)I.kp_begin + I.kp_count > n_kp) return OKVIS_BA_ERR_ARG;
    for (int k = I.kp_begin; k < I.kp_begin + I.kp_count; ++k)
      if (!std::isfinite(kp[3 * (size_t)k]) || !std::isfinite(kp[3 * (size_t)k + 1])) return OKVIS_BA_ERR_ARG;
    n_hull += (size_t)I.kp_count;
    n_max = std::max(n_max, I.kp_count);
  }
  if (n_hull > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_kf_job& J = jobs[j];
    if (J.n_cams < 1 || J.n_cams > fe::KF_MAX_CAMS || J.im_begin < 0 || (int64_t)J.im_begin + J.n_cams > n_images || J.num_frames < 0)
      return OKVIS_BA_ERR_ARG;
  }
  if (n_images == 0) return OKVIS_BA_OK;  // then there is no job either
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  const auto s_xy = st.in<fe::KfPoint>((size_t)n_kp);
  const auto s_m = st.in<uint8_t>((size_t)n_kp);
  const auto s_table = st.in<fe::KfImage>((size_t)n_images);
  const bool want_hulls = hull_all || hull_matched;
  // the hull lists are the kernel's working memory; they come back only where a referee asks for them
  const auto s_ha_tmp = st.scratch<int32_t>(n_hull, !want_hulls), s_hm_tmp = st.scratch<int32_t>(n_hull, !want_hulls);
  const auto s_rec = st.out<fe::KfRecord>((size_t)n_images);
  const auto s_ha = want_hulls ? st.out<int32_t>(n_hull) : s_ha_tmp, s_hm = want_hulls ? st.out<int32_t>(n_hull) : s_hm_tmp;
  if (int rc = st.reserve()) return rc;
  // by hand: the size column stays behind
  fe::KfPoint* xy = st.host(s_xy);
  for (size_t k = 0; k < (size_t)n_kp; ++k) xy[k].x = kp[3 * k], xy[k].y = kp[3 * k + 1];
  if (n_kp > 0) st.put(s_m, matched);
  fe::KfImage* table = st.host(s_table);
  size_t hull0 = 0;
  for (int i = 0; i < n_images; ++i) {
    table[i] = fe::KfImage{images[i].kp_begin, images[i].kp_count, (int32_t)hull0, 0};
    hull0 += (size_t)images[i].kp_count;
  }
  if (int rc = st.upload()) return rc;
  fe::KfParams P;
  P.xy = st.dev(s_xy), P.matched = st.dev(s_m), P.images = st.dev(s_table), P.rec = st.dev(s_rec);
  P.hull_all = st.dev(s_ha), P.hull_matched = st.dev(s_hm);
  hipLaunchKernelGGL(fe::keyframe_kernel, dim3((unsigned)n_images), dim3(fe::KF_THREADS), sizeof(fe::KfPoint) * (size_t)n_max, c->stream, P);
  FE_TRY(hipGetLastError());
  if (int rc = st.download()) return rc;
  const fe::KfRecord* rec = st.host(s_rec);
  for (int i = 0; i < n_images; ++i) {
    const fe::KfRecord& R = rec[i];
    if (n_matched) n_matched[i] = R.n_matched;
    if (hull_all_size) hull_all_size[i] = R.hull_all_size;
    if (hull_matched_size) hull_matched_size[i] = R.hull_matched_size;
    if (area_all) area_all[i] = R.area_all;
    if (area_matched) area_matched[i] = R.area_matched;
    if (n_inside) n_inside[i] = R.n_inside;
    if (flags) flags[i] = (uint8_t)R.flags;
    const size_t at = (size_t)table[i].hull0, n = (size_t)table[i].n;
    if (hull_all) {
      std::copy_n(st.host(s_ha) + at, (size_t)R.hull_all_size, hull_all + at);
      std::fill(hull_all + at + R.hull_all_size, hull_all + at + n, -1);
    }
    if (hull_matched) {
      std::copy_n(st.host(s_hm) + at, (size_t)R.hull_matched_size, hull_matched + at);
      std::fill(hull_matched + at + R.hull_matched_size, hull_matched + at + n, -1);
    }
  }
  // Frontend.cpp:307-368 per job, from the records of its images
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_kf_job& J = jobs[j];
    double o, r;
    const int d = fe::kf_fold(rec + J.im_begin, J.n_cams, J.num_frames, J.initialized, J.overlap_threshold, J.ratio_threshold, &o, &r);
    if (decision) decision[j] = (uint8_t)d;
    if (overlap) overlap[j] = o;
    if (ratio) ratio[j] = r;
  }
  return OKVIS_BA_OK;
}

}  // extern "C"
