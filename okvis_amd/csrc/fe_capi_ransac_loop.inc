// Part of fe_capi.hip (one translation unit).  okvis_fe_ransac: the sampler and the loop around the solvers and the consensus
// stage of fe_capi_ransac.inc, whose helpers (SacSum, put_transposed, push_sac_job, launch_consensus) and kernels it uses as they
// are.  Five launches on one stream between one copy in and one copy back.
extern "C" {

int okvis_fe_ransac(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_ransac_job* jobs) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs)) return OKVIS_BA_ERR_ARG;
  if (n_jobs == 0) return OKVIS_BA_OK;
  struct Plan {
    Staged<double> a, b, s1, s2, cams, models;  // absolute: a points, b bearings, s1 sigma
    Staged<double> scores;  // never on: the member is here because push_sac_job's template reads p.scores (no score matrix leaves this entry)
    Staged<int32_t> ci, samples, inliers;
    Staged<uint8_t> valid;
    int s = 0;
    bool live = false;  // n >= s: the job is sampled, solved, scored and looped over
  };
  struct Head {  // what push_sac_job reads of a job
    double threshold;
    int32_t kind, n, n_models;
  };
  std::vector<Plan> plan((size_t)n_jobs);
  size_t live = 0, sample_blocks = 0, solve_jobs = 0, solve_blocks = 0, gp3_jobs = 0, gp3_blocks = 0;
  SacSum total;  // of the live jobs
  bool want_counts = false;
  const auto blocks_of = [](size_t slots, size_t per) { return (slots + per - 1) / per; };
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_ransac_job& J = jobs[j];
    if (J.kind < OKVIS_FE_SAC_ABSOLUTE || J.kind > OKVIS_FE_SAC_RELATIVE || J.n < 0 || J.n > fe::SAC_MAX_N || J.n_slots < 1 ||
        J.n_slots > fe::SAC_MAX_MODELS || J.max_iterations < 1 || !(J.probability > 0.0 && J.probability < 1.0))
      return OKVIS_BA_ERR_ARG;
    if (J.kind == OKVIS_FE_SAC_ABSOLUTE) {
      if (J.n_cams < 1 || J.n_cams > fe::SAC_MAX_CAMS) return OKVIS_BA_ERR_ARG;
      if (J.n > 0 && (!J.points || !J.bearing || !J.sigma || !J.cam_index || !J.cam_offsets || !J.cam_rotations)) return OKVIS_BA_ERR_ARG;
      for (int i = 0; i < J.n; ++i)
        if (J.cam_index[i] < 0 || J.cam_index[i] >= J.n_cams) return OKVIS_BA_ERR_ARG;
    } else if (J.n > 0 && (!J.bearing1 || !J.bearing2 || !J.sigma1 || !J.sigma2)) {
      return OKVIS_BA_ERR_ARG;
    }
    Plan& p = plan[j];
    p.s = fe::sac_sample_size(J.kind), p.live = J.n >= p.s;
    if (!p.live) continue;
    ++live, sample_blocks += blocks_of((size_t)J.n_slots, fe::SAC_SAMPLE_THREADS);
    if (J.kind == OKVIS_FE_SAC_ABSOLUTE) ++gp3_jobs, gp3_blocks += blocks_of((size_t)J.n_slots, fe::GP3_PER_WAVE);
    else ++solve_jobs, solve_blocks += J.kind == OKVIS_FE_SAC_RELATIVE ? (size_t)J.n_slots : blocks_of((size_t)J.n_slots, 64);
    total.add(J.n, J.n_slots);
    want_counts = want_counts || J.counts;
  }
  if (sample_blocks > (size_t)INT32_MAX || solve_blocks > (size_t)INT32_MAX || gp3_blocks > (size_t)INT32_MAX || live > (size_t)INT32_MAX ||
      !total.launchable())
    return OKVIS_BA_ERR_ARG;
  Stage st{c};
  Staged<fe::LoopRecord> s_rec;
  if (live > 0) {
    FE_TRY(hipSetDevice(c->device));
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_ransac_job& J = jobs[j];
      Plan& p = plan[j];
      if (!p.live) continue;
      const size_t n = (size_t)J.n;
      const bool absolute = J.kind == OKVIS_FE_SAC_ABSOLUTE;
      p.a = st.in<double>(3 * n), p.b = st.in<double>(3 * n), p.s1 = st.in<double>(n), p.s2 = st.in<double>(n, !absolute);
      p.ci = st.in<int32_t>(n, absolute), p.cams = st.in<double>(12 * (size_t)J.n_cams, absolute);
    }
    const auto s_sample = st.in<fe::SampleJob>(live);
    const auto s_solve = st.in<fe::SolveJob>(solve_jobs, solve_jobs > 0);
    const auto s_gp3 = st.in<fe::Gp3Job>(gp3_jobs, gp3_jobs > 0);
    const auto s_table = st.in<fe::SacJob>(live);
    const auto s_loop = st.in<fe::LoopJob>(live);
    const auto width = [&](int j) { return (size_t)(jobs[j].kind == OKVIS_FE_SAC_ROTATION_ONLY ? 9 : 12); };
    // what the caller does not take stays on the device: samples, validity, hypotheses, counts, ballots
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_ransac_job& J = jobs[j];
      Plan& p = plan[j];
      if (!p.live) continue;
      if (!J.samples) p.samples = st.scratch<int32_t>((size_t)J.n_slots * (size_t)p.s);
      if (!J.valid) p.valid = st.scratch<uint8_t>((size_t)J.n_slots);
      if (!J.models) p.models = st.scratch<double>((size_t)J.n_slots * width(j));
    }
    // the counts of all jobs are ONE array (launch_consensus zeroes it and the kernel indexes it by count0): it is scratch, unless any
    // job asks for its referee counts, which makes the whole array an output, copied back for every job and handed out to those that asked
    Staged<int32_t> s_counts;
    if (!want_counts) s_counts = st.scratch<int32_t>(total.counts);
    const auto s_ballots = st.scratch<unsigned long long>(total.words);
    s_rec = st.out<fe::LoopRecord>(live);
    for (int j = 0; j < n_jobs; ++j)
      if (plan[j].live) plan[j].inliers = st.out<int32_t>((size_t)jobs[j].n, jobs[j].inliers != nullptr);
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_ransac_job& J = jobs[j];
      Plan& p = plan[j];
      if (!p.live) continue;
      if (J.samples) p.samples = st.out<int32_t>((size_t)J.n_slots * (size_t)p.s);
      if (J.valid) p.valid = st.out<uint8_t>((size_t)J.n_slots);
      if (J.models) p.models = st.out<double>((size_t)J.n_slots * width(j));
    }
    if (want_counts) s_counts = st.out<int32_t>(total.counts);
    if (int rc = st.reserve()) return rc;
    fe::SampleJob* sample_table = st.host(s_sample);
    fe::SolveJob* solve_table = st.host(s_solve);
    fe::Gp3Job* gp3_table = st.host(s_gp3);
    fe::SacJob* table = st.host(s_table);
    fe::LoopJob* loop_table = st.host(s_loop);
    fe::LoopRecord* records = st.dev(s_rec);
    size_t sample_block0 = 0, solve_block0 = 0, gp3_block0 = 0;
    SacSum at;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_ransac_job& J = jobs[j];
      const Plan& p = plan[j];
      if (!p.live) continue;
      const bool absolute = J.kind == OKVIS_FE_SAC_ABSOLUTE;
      put_transposed(st, p.a, absolute ? J.points : J.bearing1), put_transposed(st, p.b, absolute ? J.bearing : J.bearing2);
      st.put(p.s1, absolute ? J.sigma : J.sigma1), st.put(p.s2, J.sigma2), st.put(p.ci, J.cam_index);
      fe::SampleJob Q;
      Q.samples = st.dev(p.samples), Q.seed = J.seed, Q.n = J.n, Q.n_slots = J.n_slots, Q.s = p.s, Q.block0 = (int32_t)sample_block0;
      *sample_table++ = Q, sample_block0 += blocks_of((size_t)J.n_slots, fe::SAC_SAMPLE_THREADS);
      if (absolute) {
        double* cams = st.host(p.cams);
        for (int k = 0; k < J.n_cams; ++k) {
          std::copy_n(J.cam_offsets + 3 * k, 3, cams + 12 * k);
          std::copy_n(J.cam_rotations + 9 * k, 9, cams + 12 * k + 3);
        }
        fe::Gp3Job S;
        S.points = st.dev(p.a), S.bearing = st.dev(p.b), S.cam_index = st.dev(p.ci), S.cams = st.dev(p.cams), S.samples = st.dev(p.samples);
        S.models = st.dev(p.models), S.valid = st.dev(p.valid), S.n_roots = nullptr, S.candidates = nullptr;
        S.n = J.n, S.n_models = J.n_slots, S.block0 = (int32_t)gp3_block0;
        *gp3_table++ = S, gp3_block0 += blocks_of((size_t)J.n_slots, fe::GP3_PER_WAVE);
      } else {
        fe::SolveJob S;
        S.a = st.dev(p.a), S.b = st.dev(p.b), S.sigma1 = st.dev(p.s1), S.sigma2 = st.dev(p.s2), S.samples = st.dev(p.samples);
        S.models = st.dev(p.models), S.valid = st.dev(p.valid), S.n_roots = nullptr, S.essentials = nullptr;
        S.kind = J.kind, S.n = J.n, S.n_models = J.n_slots, S.block0 = (int32_t)solve_block0;
        *solve_table++ = S, solve_block0 += J.kind == OKVIS_FE_SAC_RELATIVE ? (size_t)J.n_slots : blocks_of((size_t)J.n_slots, 64);
      }
      fe::LoopJob L;
      L.counts = st.dev(s_counts) + at.counts, L.valid = st.dev(p.valid), L.ballots = st.dev(s_ballots) + at.words;
      L.models = st.dev(p.models), L.inliers = st.dev(p.inliers), L.record = records++;
      L.probability = J.probability, L.n = J.n, L.n_slots = J.n_slots, L.s = p.s, L.max_iterations = J.max_iterations;
      L.width = J.kind == OKVIS_FE_SAC_ROTATION_ONLY ? 9 : 12;
      *loop_table++ = L;
      push_sac_job(st, table, at, Head{J.threshold, J.kind, J.n, J.n_slots}, p, st.dev(p.ci), st.dev(p.cams));
    }
    if (int rc = st.upload()) return rc;
    fe::SampleParams QP;
    QP.jobs = st.dev(s_sample), QP.n_jobs = (int32_t)live;
    hipLaunchKernelGGL(fe::sac_sample_kernel, dim3((unsigned)sample_blocks), dim3(fe::SAC_SAMPLE_THREADS), 0, c->stream, QP);
    FE_TRY(hipGetLastError());
    if (solve_jobs > 0) {
      fe::SolveParams SP;
      SP.jobs = st.dev(s_solve), SP.n_jobs = (int32_t)solve_jobs;
      hipLaunchKernelGGL(fe::sac_solve_kernel, dim3((unsigned)solve_blocks), dim3(64), 0, c->stream, SP);
      FE_TRY(hipGetLastError());
    }
    if (gp3_jobs > 0) {
      fe::Gp3Params GP;
      GP.jobs = st.dev(s_gp3), GP.n_jobs = (int32_t)gp3_jobs;
      hipLaunchKernelGGL(fe::sac_gp3p_kernel, dim3((unsigned)gp3_blocks), dim3(64), 0, c->stream, GP);
      FE_TRY(hipGetLastError());
    }
    if (int rc = launch_consensus(st, s_table, total, s_counts, s_ballots)) return rc;
    fe::LoopParams LP;
    LP.jobs = st.dev(s_loop), LP.n_jobs = (int32_t)live;
    hipLaunchKernelGGL(fe::sac_loop_kernel, dim3((unsigned)live), dim3(64), 0, c->stream, LP);
    FE_TRY(hipGetLastError());
    if (int rc = st.download()) return rc;
    const fe::LoopRecord* rec = st.host(s_rec);
    at = SacSum();
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_ransac_job& J = jobs[j];
      const Plan& p = plan[j];
      if (!p.live) continue;
      const fe::LoopRecord& R = *rec++;
      if (J.best) *J.best = R.best;
      if (J.n_inliers) *J.n_inliers = R.n_inliers;
      if (J.iterations) *J.iterations = R.iterations;
      if (J.skipped) *J.skipped = R.skipped;
      if (J.stop) *J.stop = R.stop;
      if (J.model) std::copy_n(R.model, J.kind == OKVIS_FE_SAC_ROTATION_ONLY ? 9 : 12, J.model);
      if (J.inliers) std::copy_n(st.host(p.inliers), R.n_inliers, J.inliers);
      if (J.samples) st.get(p.samples, J.samples);
      if (J.valid) st.get(p.valid, J.valid);
      if (J.models) st.get(p.models, J.models);
      if (J.counts) std::copy_n(st.host(s_counts) + at.counts, J.n_slots, J.counts);
      at.add(J.n, J.n_slots);
    }
  }
  for (int j = 0; j < n_jobs; ++j) {  // n below the sample size: nothing was launched
    const okvis_fe_ransac_job& J = jobs[j];
    if (plan[j].live) continue;
    if (J.best) *J.best = -1;
    if (J.n_inliers) *J.n_inliers = 0;
    if (J.iterations) *J.iterations = 0;
    if (J.skipped) *J.skipped = 0;
    if (J.stop) *J.stop = OKVIS_FE_RANSAC_STOP_NO_SAMPLE;
    if (J.model) std::fill_n(J.model, J.kind == OKVIS_FE_SAC_ROTATION_ONLY ? 9 : 12, fe::sac_nan());
  }
  return OKVIS_BA_OK;
}

}  // extern "C"
