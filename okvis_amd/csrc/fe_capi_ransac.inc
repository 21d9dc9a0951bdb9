// Part of fe_capi.hip (one translation unit).  Bearing vectors, consensus scoring and the minimal solvers in front of it.  The
// consensus stage (what a scored job adds to the launch, its device record, the launch, Ransac::computeModel's book-keeping) is
// written once and serves okvis_fe_sac_consensus, okvis_fe_sac_solve and okvis_fe_sac_solve_absolute, templated on the job type
// where the fields carry the same names.
namespace {

// What the scored jobs of a call take of sac_consensus_kernel's grid and of its two result arrays, summed job by job: the sums
// over the jobs before a job are its first block, count and ballot word.  The only place these formulas stand.
struct SacSum {
  size_t jobs = 0, blocks = 0, counts = 0, words = 0;
  static size_t tiles(int32_t n) { return ((size_t)n + fe::SAC_THREADS - 1) / fe::SAC_THREADS; }
  static size_t row_words(int32_t n) { return ((size_t)n + 63) / 64; }  // ballot words of one hypothesis
  void add(int32_t n, int32_t n_models) {
    ++jobs, blocks += tiles(n) * (((size_t)n_models + fe::SAC_MODEL_TILE - 1) / fe::SAC_MODEL_TILE);
    counts += (size_t)n_models, words += (size_t)n_models * row_words(n);
  }
  bool launchable() const { return blocks <= (size_t)INT32_MAX && counts <= (size_t)INT32_MAX; }
};

// src [n][3] goes to the device as [3][n], so that a wave reads 64 consecutive doubles
void put_transposed(const Stage& st, const Staged<double>& a, const double* src) {
  double* dst = st.host(a);
  const size_t n = a.n / 3;
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) dst[k * n + i] = src[3 * i + k];
}

// the device record of scored job J, whose arrays are staged as plan p says (models, a, b, s1, s2, scores), behind the jobs of `at`
template <class Job, class Plan>
void push_sac_job(const Stage& st, fe::SacJob*& table, SacSum& at, const Job& J, const Plan& p, const int32_t* cam_index, const double* cams) {
  fe::SacJob D;
  D.models = st.dev(p.models), D.a = st.dev(p.a), D.b = st.dev(p.b), D.sigma1 = st.dev(p.s1), D.sigma2 = st.dev(p.s2);
  D.cam_index = cam_index, D.cams = cams, D.scores = st.dev(p.scores);
  D.threshold = J.threshold, D.kind = J.kind, D.n = J.n, D.n_models = J.n_models;
  D.block0 = (int32_t)at.blocks, D.tiles = (int32_t)SacSum::tiles(J.n), D.count0 = (int32_t)at.counts, D.word0 = (int64_t)at.words;
  *table++ = D, at.add(J.n, J.n_models);
}

// sac_consensus_kernel over the `total` of the jobs in `table`, the counts zeroed in front of it
int launch_consensus(const Stage& st, const Staged<fe::SacJob>& table, const SacSum& total, const Staged<int32_t>& counts,
                     const Staged<unsigned long long>& ballots) {
  FE_TRY(hipMemsetAsync(st.dev(counts), 0, counts.bytes(), st.c->stream));
  fe::SacParams P;
  P.jobs = st.dev(table), P.n_jobs = (int32_t)total.jobs;
  P.counts = st.dev(counts), P.ballots = st.dev(ballots);
  hipLaunchKernelGGL(fe::sac_consensus_kernel, dim3((unsigned)total.blocks), dim3(fe::SAC_THREADS), 0, st.c->stream, P);
  FE_TRY(hipGetLastError());
  return OKVIS_BA_OK;
}

// Ransac::computeModel's book-keeping of scored job J, behind the jobs of `at`, on its counts (a hypothesis replaces the best only
// with strictly more inliers); the best hypothesis's row of ballot words expanded into indices; the score matrix where it came back
template <class Job>
void sac_book_keeping(const Stage& st, SacSum& at, const Staged<int32_t>& s_counts, const Staged<unsigned long long>& s_ballots, const Job& J,
                      const Staged<double>& scores) {
  const size_t words = SacSum::row_words(J.n);
  const int32_t* counts = st.host(s_counts) + at.counts;
  const unsigned long long* ballots = st.host(s_ballots) + at.words;
  at.add(J.n, J.n_models);
  int best = 0;
  for (int m = 1; m < J.n_models; ++m)
    if (counts[m] > counts[best]) best = m;
  if (J.counts) std::copy_n(counts, J.n_models, J.counts);
  if (J.best) *J.best = best;
  if (J.n_inliers) *J.n_inliers = counts[best];
  if (J.inliers) {
    int32_t k = 0;
    for (size_t w = 0; w < words; ++w)
      for (unsigned long long m = ballots[(size_t)best * words + w]; m; m &= m - 1) J.inliers[k++] = (int32_t)(64 * w) + __builtin_ctzll(m);
  }
  st.get(scores, J.scores);
}

}  // namespace

extern "C" {

int okvis_fe_bearing_vectors(okvis_fe_context* c, const okvis_fe_camera* cam, int32_t n, const float* kp, double* bearing,
                             double* sigma_angle, uint8_t* ok) {
  if (!c || !camera_ok(cam) || n < 0) return OKVIS_BA_ERR_ARG;
  if (n == 0) return OKVIS_BA_OK;
  if (!kp) return OKVIS_BA_ERR_ARG;
  fe::BearingParams P;
  P.cam = to_device(cam), P.n = n;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  const auto s_kp = st.in<float>(3 * (size_t)n);
  const auto s_b = st.out<double>(3 * (size_t)n), s_s = st.out<double>((size_t)n);
  const auto s_ok = st.out<uint8_t>((size_t)n);
  if (int rc = st.reserve()) return rc;
  st.put(s_kp, kp);
  if (int rc = st.upload()) return rc;
  P.kp = st.dev(s_kp), P.bearing = st.dev(s_b), P.sigma = st.dev(s_s), P.ok = st.dev(s_ok);
  hipLaunchKernelGGL(fe::bearing_vectors_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, P);
  FE_TRY(hipGetLastError());
  if (int rc = st.download()) return rc;
  st.get(s_b, bearing), st.get(s_s, sigma_angle), st.get(s_ok, ok);
  return OKVIS_BA_OK;
}

int okvis_fe_sac_consensus(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_sac_job* jobs) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs)) return OKVIS_BA_ERR_ARG;
  SacSum total;  // of the jobs with correspondences
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_job& J = jobs[j];
    if (J.kind < OKVIS_FE_SAC_ABSOLUTE || J.kind > OKVIS_FE_SAC_RELATIVE || J.n < 0 || J.n > fe::SAC_MAX_N || J.n_models < 1 ||
        J.n_models > fe::SAC_MAX_MODELS || !J.models)
      return OKVIS_BA_ERR_ARG;
    if (J.kind == OKVIS_FE_SAC_ABSOLUTE) {
      if (J.n_cams < 1 || J.n_cams > fe::SAC_MAX_CAMS) return OKVIS_BA_ERR_ARG;
      if (J.n > 0 && (!J.points || !J.bearing || !J.sigma || !J.cam_index || !J.cam_offsets || !J.cam_rotations)) return OKVIS_BA_ERR_ARG;
      for (int i = 0; i < J.n; ++i)
        if (J.cam_index[i] < 0 || J.cam_index[i] >= J.n_cams) return OKVIS_BA_ERR_ARG;
    } else if (J.n > 0 && (!J.bearing1 || !J.bearing2 || !J.sigma1 || !J.sigma2)) {
      return OKVIS_BA_ERR_ARG;
    }
    if (J.n > 0) total.add(J.n, J.n_models);
  }
  if (!total.launchable()) return OKVIS_BA_ERR_ARG;
  Stage st{c};
  Staged<int32_t> s_counts;
  Staged<unsigned long long> s_ballots;
  struct Plan {
    Staged<double> models, a, b, s1, s2, cams, scores;
    Staged<int32_t> ci;
  };
  std::vector<Plan> plan((size_t)n_jobs);
  if (total.jobs > 0) {
    FE_TRY(hipSetDevice(c->device));
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_sac_job& J = jobs[j];
      if (J.n == 0) continue;
      Plan& p = plan[j];
      const size_t n = (size_t)J.n;
      const bool absolute = J.kind == OKVIS_FE_SAC_ABSOLUTE;
      p.models = st.in<double>((size_t)(J.kind == OKVIS_FE_SAC_ROTATION_ONLY ? 9 : 12) * J.n_models);
      p.a = st.in<double>(3 * n), p.b = st.in<double>(3 * n), p.s1 = st.in<double>(n), p.s2 = st.in<double>(n, !absolute);
      p.ci = st.in<int32_t>(n, absolute), p.cams = st.in<double>(12 * (size_t)J.n_cams, absolute);
    }
    const auto s_table = st.in<fe::SacJob>(total.jobs);
    s_counts = st.out<int32_t>(total.counts), s_ballots = st.out<unsigned long long>(total.words);
    for (int j = 0; j < n_jobs; ++j)  // a score matrix comes back only where a job asked for it
      plan[j].scores = st.out<double>((size_t)jobs[j].n_models * (size_t)jobs[j].n, jobs[j].n > 0 && jobs[j].scores);
    if (int rc = st.reserve()) return rc;
    fe::SacJob* table = st.host(s_table);
    SacSum at;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_sac_job& J = jobs[j];
      if (J.n == 0) continue;
      const bool absolute = J.kind == OKVIS_FE_SAC_ABSOLUTE;
      const Plan& p = plan[j];
      st.put(p.models, J.models);
      put_transposed(st, p.a, absolute ? J.points : J.bearing1), put_transposed(st, p.b, absolute ? J.bearing : J.bearing2);
      st.put(p.s1, absolute ? J.sigma : J.sigma1), st.put(p.s2, J.sigma2), st.put(p.ci, J.cam_index);
      if (absolute) {
        double* cams = st.host(p.cams);
        for (int k = 0; k < J.n_cams; ++k) {
          std::copy_n(J.cam_offsets + 3 * k, 3, cams + 12 * k);
          std::copy_n(J.cam_rotations + 9 * k, 9, cams + 12 * k + 3);
        }
      }
      push_sac_job(st, table, at, J, p, st.dev(p.ci), st.dev(p.cams));
    }
    if (int rc = st.upload()) return rc;
    if (int rc = launch_consensus(st, s_table, total, s_counts, s_ballots)) return rc;
    if (int rc = st.download()) return rc;
  }
  SacSum at;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_job& J = jobs[j];
    if (J.n == 0) {
      if (J.counts) std::fill_n(J.counts, J.n_models, 0);
      if (J.best) *J.best = 0;
      if (J.n_inliers) *J.n_inliers = 0;
      continue;
    }
    sac_book_keeping(st, at, s_counts, s_ballots, J, plan[j].scores);
  }
  return OKVIS_BA_OK;
}

// The solvers in front of the consensus kernel: one staging copy in, sac_solve_kernel for all jobs, the consensus stage on the
// hypotheses where the solver left them, one copy back.
int okvis_fe_sac_solve(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_sac_solve_job* jobs) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs)) return OKVIS_BA_ERR_ARG;
  if (n_jobs == 0) return OKVIS_BA_OK;
  struct Plan {
    Staged<double> a, b, s1, s2, models, essentials, scores;
    Staged<int32_t> samples, n_roots;
    Staged<uint8_t> valid;
    bool scored = false;  // a consensus output is asked for
  };
  std::vector<Plan> plan((size_t)n_jobs);
  size_t solve_blocks = 0;
  SacSum total;  // of the scored jobs
  const auto job_solve_blocks = [](const okvis_fe_sac_solve_job& J) {
    return J.kind == OKVIS_FE_SAC_RELATIVE ? (size_t)J.n_models : ((size_t)J.n_models + 63) / 64;
  };
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_solve_job& J = jobs[j];
    if ((J.kind != OKVIS_FE_SAC_ROTATION_ONLY && J.kind != OKVIS_FE_SAC_RELATIVE) || J.n < 0 || J.n > fe::SAC_MAX_N || J.n_models < 1 ||
        J.n_models > fe::SAC_MAX_MODELS || !J.samples || (J.n > 0 && (!J.bearing1 || !J.bearing2)))
      return OKVIS_BA_ERR_ARG;
    plan[j].scored = J.counts || J.best || J.n_inliers || J.inliers || J.scores;
    if (plan[j].scored && (!J.sigma1 || !J.sigma2)) return OKVIS_BA_ERR_ARG;
    const size_t width = J.kind == OKVIS_FE_SAC_RELATIVE ? OKVIS_FE_SAC_SAMPLE_RELATIVE : OKVIS_FE_SAC_SAMPLE_ROTATION_ONLY;
    for (size_t i = 0; i < width * (size_t)J.n_models; ++i)
      if (J.samples[i] < 0 || J.samples[i] >= J.n) return OKVIS_BA_ERR_ARG;  // n = 0 ends here: every job past this line has n >= 1
    solve_blocks += job_solve_blocks(J);
    if (plan[j].scored) total.add(J.n, J.n_models);
  }
  if (solve_blocks > (size_t)INT32_MAX || !total.launchable()) return OKVIS_BA_ERR_ARG;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_solve_job& J = jobs[j];
    Plan& p = plan[j];
    const size_t n = (size_t)J.n;
    p.a = st.in<double>(3 * n), p.b = st.in<double>(3 * n);
    p.s1 = st.in<double>(n, J.sigma1 != nullptr), p.s2 = st.in<double>(n, J.sigma2 != nullptr);
    p.samples = st.in<int32_t>((size_t)J.n_models * (J.kind == OKVIS_FE_SAC_RELATIVE ? 8 : 2));
  }
  const auto s_solve = st.in<fe::SolveJob>((size_t)n_jobs);
  const auto s_table = st.in<fe::SacJob>(total.jobs, total.jobs > 0);
  const auto model_doubles = [&](int j) { return (size_t)jobs[j].n_models * (jobs[j].kind == OKVIS_FE_SAC_RELATIVE ? 12 : 9); };
  for (int j = 0; j < n_jobs; ++j)  // hypotheses the caller does not take stay on the device
    if (!jobs[j].models) plan[j].models = st.scratch<double>(model_doubles(j));
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_solve_job& J = jobs[j];
    const bool relative = J.kind == OKVIS_FE_SAC_RELATIVE;
    if (J.models) plan[j].models = st.out<double>(model_doubles(j));
    plan[j].valid = st.out<uint8_t>((size_t)J.n_models, J.valid != nullptr);
    plan[j].n_roots = st.out<int32_t>((size_t)J.n_models, relative && J.n_roots);
    plan[j].essentials = st.out<double>(90 * (size_t)J.n_models, relative && J.essentials);
  }
  const auto s_counts = st.out<int32_t>(total.counts, total.jobs > 0);
  const auto s_ballots = st.out<unsigned long long>(total.words, total.jobs > 0);
  for (int j = 0; j < n_jobs; ++j) plan[j].scores = st.out<double>((size_t)jobs[j].n_models * (size_t)jobs[j].n, jobs[j].scores != nullptr);
  if (int rc = st.reserve()) return rc;
  fe::SolveJob* solve_table = st.host(s_solve);
  fe::SacJob* table = st.host(s_table);
  size_t solve_block0 = 0;
  SacSum at;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_solve_job& J = jobs[j];
    const Plan& p = plan[j];
    put_transposed(st, p.a, J.bearing1), put_transposed(st, p.b, J.bearing2);  // as the consensus kernel reads them
    st.put(p.s1, J.sigma1), st.put(p.s2, J.sigma2), st.put(p.samples, J.samples);
    fe::SolveJob S;
    S.a = st.dev(p.a), S.b = st.dev(p.b), S.sigma1 = st.dev(p.s1), S.sigma2 = st.dev(p.s2), S.samples = st.dev(p.samples);
    S.models = st.dev(p.models), S.valid = st.dev(p.valid), S.n_roots = st.dev(p.n_roots), S.essentials = st.dev(p.essentials);
    S.kind = J.kind, S.n = J.n, S.n_models = J.n_models, S.block0 = (int32_t)solve_block0;
    solve_table[j] = S;
    solve_block0 += job_solve_blocks(J);
    if (p.scored) push_sac_job(st, table, at, J, p, nullptr, nullptr);
  }
  if (int rc = st.upload()) return rc;
  // essentials past n_roots are not written by the kernel: NaN, so that the copy back never hands out stale staging bytes
  for (int j = 0; j < n_jobs; ++j)
    if (plan[j].essentials.on) FE_TRY(hipMemsetAsync(st.dev(plan[j].essentials), 0xff, plan[j].essentials.bytes(), c->stream));
  fe::SolveParams SP;
  SP.jobs = st.dev(s_solve), SP.n_jobs = n_jobs;
  hipLaunchKernelGGL(fe::sac_solve_kernel, dim3((unsigned)solve_blocks), dim3(64), 0, c->stream, SP);
  FE_TRY(hipGetLastError());
  if (total.jobs > 0)
    if (int rc = launch_consensus(st, s_table, total, s_counts, s_ballots)) return rc;
  if (int rc = st.download()) return rc;
  at = SacSum();
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_solve_job& J = jobs[j];
    const Plan& p = plan[j];
    if (J.models) st.get(p.models, J.models);
    st.get(p.valid, J.valid), st.get(p.n_roots, J.n_roots), st.get(p.essentials, J.essentials);
    if (p.scored) sac_book_keeping(st, at, s_counts, s_ballots, J, p.scores);
  }
  return OKVIS_BA_OK;
}

// The 3D-2D solver in front of the consensus kernel, as okvis_fe_sac_solve: one staging copy in, sac_gp3p_kernel for all jobs, the
// consensus stage on the hypotheses where the solver left them and on the points, bearings and cameras as the solver read them,
// one copy back.
int okvis_fe_sac_solve_absolute(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_sac_absolute_job* jobs) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs)) return OKVIS_BA_ERR_ARG;
  if (n_jobs == 0) return OKVIS_BA_OK;
  struct Plan {
    Staged<double> a, b, s1, s2, cams, models, candidates, scores;  // a: points, b: bearings, s1: sigma, s2: never on
    Staged<int32_t> ci, samples, n_roots;
    Staged<uint8_t> valid;
    bool scored = false;  // a consensus output is asked for
  };
  struct Head {  // what push_sac_job reads of a job
    double threshold;
    int32_t kind, n, n_models;
  };
  std::vector<Plan> plan((size_t)n_jobs);
  size_t solve_blocks = 0;
  SacSum total;  // of the scored jobs
  const auto job_solve_blocks = [](const okvis_fe_sac_absolute_job& J) { return ((size_t)J.n_models + fe::GP3_PER_WAVE - 1) / fe::GP3_PER_WAVE; };
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_absolute_job& J = jobs[j];
    if (J.n < 0 || J.n > fe::SAC_MAX_N || J.n_models < 1 || J.n_models > fe::SAC_MAX_MODELS || J.n_cams < 1 || J.n_cams > fe::SAC_MAX_CAMS ||
        !J.samples || (J.n > 0 && (!J.points || !J.bearing || !J.cam_index || !J.cam_offsets || !J.cam_rotations)))
      return OKVIS_BA_ERR_ARG;
    plan[j].scored = J.counts || J.best || J.n_inliers || J.inliers || J.scores;
    if (plan[j].scored && !J.sigma) return OKVIS_BA_ERR_ARG;
    for (int i = 0; i < J.n; ++i)
      if (J.cam_index[i] < 0 || J.cam_index[i] >= J.n_cams) return OKVIS_BA_ERR_ARG;
    for (size_t i = 0; i < (size_t)OKVIS_FE_SAC_SAMPLE_ABSOLUTE * (size_t)J.n_models; ++i)
      if (J.samples[i] < 0 || J.samples[i] >= J.n) return OKVIS_BA_ERR_ARG;  // n = 0 ends here: every job past this line has n >= 1
    solve_blocks += job_solve_blocks(J);
    if (plan[j].scored) total.add(J.n, J.n_models);
  }
  if (solve_blocks > (size_t)INT32_MAX || !total.launchable()) return OKVIS_BA_ERR_ARG;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_absolute_job& J = jobs[j];
    Plan& p = plan[j];
    const size_t n = (size_t)J.n;
    p.a = st.in<double>(3 * n), p.b = st.in<double>(3 * n), p.s1 = st.in<double>(n, J.sigma != nullptr);
    p.ci = st.in<int32_t>(n), p.cams = st.in<double>(12 * (size_t)J.n_cams);
    p.samples = st.in<int32_t>((size_t)J.n_models * OKVIS_FE_SAC_SAMPLE_ABSOLUTE);
  }
  const auto s_solve = st.in<fe::Gp3Job>((size_t)n_jobs);
  const auto s_table = st.in<fe::SacJob>(total.jobs, total.jobs > 0);
  for (int j = 0; j < n_jobs; ++j)  // hypotheses the caller does not take stay on the device
    if (!jobs[j].models) plan[j].models = st.scratch<double>(12 * (size_t)jobs[j].n_models);
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_absolute_job& J = jobs[j];
    if (J.models) plan[j].models = st.out<double>(12 * (size_t)J.n_models);
    plan[j].valid = st.out<uint8_t>((size_t)J.n_models, J.valid != nullptr);
    plan[j].n_roots = st.out<int32_t>((size_t)J.n_models, J.n_roots != nullptr);
    plan[j].candidates = st.out<double>(12 * (size_t)fe::GP3_MAX_ROOTS * (size_t)J.n_models, J.candidates != nullptr);
  }
  const auto s_counts = st.out<int32_t>(total.counts, total.jobs > 0);
  const auto s_ballots = st.out<unsigned long long>(total.words, total.jobs > 0);
  for (int j = 0; j < n_jobs; ++j) plan[j].scores = st.out<double>((size_t)jobs[j].n_models * (size_t)jobs[j].n, jobs[j].scores != nullptr);
  if (int rc = st.reserve()) return rc;
  fe::Gp3Job* solve_table = st.host(s_solve);
  fe::SacJob* table = st.host(s_table);
  size_t solve_block0 = 0;
  SacSum at;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_absolute_job& J = jobs[j];
    const Plan& p = plan[j];
    put_transposed(st, p.a, J.points), put_transposed(st, p.b, J.bearing);  // as the consensus kernel reads them
    st.put(p.s1, J.sigma), st.put(p.ci, J.cam_index), st.put(p.samples, J.samples);
    double* cams = st.host(p.cams);
    for (int k = 0; k < J.n_cams; ++k) {
      std::copy_n(J.cam_offsets + 3 * k, 3, cams + 12 * k);
      std::copy_n(J.cam_rotations + 9 * k, 9, cams + 12 * k + 3);
    }
    fe::Gp3Job S;
    S.points = st.dev(p.a), S.bearing = st.dev(p.b), S.cam_index = st.dev(p.ci), S.cams = st.dev(p.cams), S.samples = st.dev(p.samples);
    S.models = st.dev(p.models), S.valid = st.dev(p.valid), S.n_roots = st.dev(p.n_roots), S.candidates = st.dev(p.candidates);
    S.n = J.n, S.n_models = J.n_models, S.block0 = (int32_t)solve_block0;
    solve_table[j] = S;
    solve_block0 += job_solve_blocks(J);
    if (p.scored) push_sac_job(st, table, at, Head{J.threshold, OKVIS_FE_SAC_ABSOLUTE, J.n, J.n_models}, p, st.dev(p.ci), st.dev(p.cams));
  }
  if (int rc = st.upload()) return rc;
  fe::Gp3Params GP;
  GP.jobs = st.dev(s_solve), GP.n_jobs = n_jobs;
  hipLaunchKernelGGL(fe::sac_gp3p_kernel, dim3((unsigned)solve_blocks), dim3(64), 0, c->stream, GP);  // writes every candidate slot: NaN past n_roots
  FE_TRY(hipGetLastError());
  if (total.jobs > 0)
    if (int rc = launch_consensus(st, s_table, total, s_counts, s_ballots)) return rc;
  if (int rc = st.download()) return rc;
  at = SacSum();
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_absolute_job& J = jobs[j];
    const Plan& p = plan[j];
    if (J.models) st.get(p.models, J.models);
    st.get(p.valid, J.valid), st.get(p.n_roots, J.n_roots), st.get(p.candidates, J.candidates);
    if (p.scored) sac_book_keeping(st, at, s_counts, s_ballots, J, p.scores);
  }
  return OKVIS_BA_OK;
}

}  // extern "C"
