// Part of fe_capi.hip (one translation unit).  Hamming candidates, descriptor matching and verified matching, with the host side
// of DenseMatcher (the assignment chains and matchBody's final loop) that the two matching entries share.
namespace {

bool desc_bytes_ok(int32_t n) { return n == 16 || n == 32 || n == 48 || n == 64; }
constexpr int32_t MATCH_MAX_KEYPOINTS = 65536;

// f(std::integral_constant<int, W>) for a descriptor of W x 16 bytes
template <class F>
void with_words(int words, F f) {
  switch (words) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, 4>()); break;
  }
}

// workgroups of hamming_rows_kernel / best_lists_kernel / verified_lists_kernel over n_a rows, one row to a wave
size_t match_blocks(int32_t n_a) { return ((size_t)n_a + fe::MATCH_WAVES - 1) / fe::MATCH_WAVES; }

template <bool WRITE>
void launch_hamming_rows(int words, const fe::CandParams& P, hipStream_t stream) {
  const dim3 grid((unsigned)match_blocks(P.n_a)), block(fe::MATCH_THREADS);
  with_words(words, [&](auto w) { hipLaunchKernelGGL((fe::hamming_rows_kernel<w(), WRITE>), grid, block, 0, stream, P); });
}

// workgroups of vmatch_prepass_kernel for one job: a lane per keypoint of A, and per keypoint of B where B has rays to form
size_t prepass_blocks(const okvis_fe_vmatch_job& J) {
  return ((size_t)J.n_a + (J.kind == OKVIS_FE_MATCH_2D2D ? (size_t)J.n_b : 0) + fe::VMATCH_PRE_THREADS - 1) / fe::VMATCH_PRE_THREADS;
}

// what fe::BestParams and fe::VListParams have in common besides their tables: the settings of the lists and where they go
template <class Params>
void fill_list_params(Params& P, const Stage& st, float threshold, int32_t num_best, int32_t use_ratio, const Staged<int32_t>& lidx,
                      const Staged<float>& ldist) {
  P.threshold = threshold, P.initial = use_ratio ? FLT_MAX : threshold, P.num_best = num_best;
  P.list_idx = st.dev(lidx), P.list_dist = st.dev(ldist);
}

// raySigmasA_ / raySigmasB_ of doSetup (VioKeyframeWindowMatchingAlgorithm.cpp:210-221, :251-261) in the reference's operation
// order; products and quotients only, so the host and any IEEE device give the same bits
double ray_sigma(float size, double fu) {
  const double sd = 0.8 * (double)size / 12.0;
  return std::sqrt(std::sqrt(2.0)) * sd / fu;
}

// DenseMatcher::assignbest (okvis_matcher/src/DenseMatcher.cpp:69-111) for row a, its recursion written as a loop: a taker has to
// be strictly better than the holder, and the holder it displaces goes on from position 1 of its own list
void assign_best(int a, int num_best, const int32_t* list_idx, const float* list_dist, int32_t* pair_a, float* pair_dist) {
  int cur = a, start = 0;
  for (;;) {
    const int32_t* li = list_idx + (size_t)cur * num_best;
    const float* ld = list_dist + (size_t)cur * num_best;
    int displaced = -1;
    for (int k = start; k < num_best && li[k] != -1; ++k) {
      const int b = li[k];
      if (pair_a[b] == -1) {
        pair_a[b] = cur, pair_dist[b] = ld[k];
        return;
      }
      if (ld[k] < pair_dist[b]) {
        displaced = pair_a[b];
        pair_a[b] = cur, pair_dist[b] = ld[k];
        break;
      }
    }
    if (displaced < 0) return;
    cur = displaced, start = 1;
  }
}

// the checks the two matching entries share: of the call ...
bool match_call_ok(const okvis_fe_context* c, int32_t n_jobs, const void* jobs, int32_t desc_bytes, int32_t num_best, int32_t use_ratio) {
  return c && n_jobs >= 0 && (n_jobs == 0 || jobs) && desc_bytes_ok(desc_bytes) && num_best >= 1 && num_best <= fe::MATCH_MAX_BEST &&
         !(use_ratio && num_best < 2);
}
// ... and of one job (okvis_fe_match_job or okvis_fe_vmatch_job): its sizes, its descriptors and its three result arrays
template <class Job>
bool match_job_ok(const Job& J) {
  if (J.n_a < 0 || J.n_b < 0 || J.n_a > MATCH_MAX_KEYPOINTS || J.n_b > MATCH_MAX_KEYPOINTS) return false;
  return !(J.n_a > 0 && !J.desc_a) && !(J.n_b > 0 && (!J.desc_b || !J.pair_a || !J.pair_dist || !J.accepted));
}

// What the host does with one job's lists li / ld (its rows of list_idx / list_dist): the assignment chains (sequential by
// nature, O(n_a * num_best)) and matchBody's final loop (DenseMatcher.hpp:92-122).  accepted(b, o) is called for every b the
// loop accepts, o = the first list entry of the row it is paired with.
template <class Job, class Accepted>
void assign_and_accept(const Job& J, const int32_t* li, const float* ld, int32_t num_best, float threshold, int32_t use_ratio,
                       float ratio_threshold, Accepted accepted) {
  for (int b = 0; b < J.n_b; ++b) J.pair_a[b] = -1, J.pair_dist[b] = FLT_MAX, J.accepted[b] = 0;
  if (J.n_a == 0 || J.n_b == 0) return;
  for (int a = 0; a < J.n_a; ++a)
    if (!(J.skip_a && J.skip_a[a])) assign_best(a, num_best, li, ld, J.pair_a, J.pair_dist);
  for (int b = 0; b < J.n_b; ++b) {
    if (!(J.pair_dist[b] < threshold)) continue;
    const size_t o = (size_t)J.pair_a[b] * (size_t)num_best;
    if (use_ratio && li[o + 1] != -1) {
      const float best = ld[o], second = ld[o + 1];
      J.accepted[b] = (best == 0 || second / best > ratio_threshold) ? 1 : 0;
    } else {
      J.accepted[b] = 1;
    }
    if (J.accepted[b]) accepted(b, o);
  }
}

}  // namespace

extern "C" {

int okvis_fe_hamming_candidates(okvis_fe_context* c, int32_t desc_bytes, int32_t n_a, const uint8_t* desc_a, const uint8_t* skip_a,
                                int32_t n_b, const uint8_t* desc_b, const uint8_t* skip_b, float threshold, int32_t capacity,
                                int32_t* pairs, float* dist, int32_t* n_pairs) {
  if (!c || !desc_bytes_ok(desc_bytes) || n_a < 0 || n_b < 0 || n_a > MATCH_MAX_KEYPOINTS || n_b > MATCH_MAX_KEYPOINTS || capacity < 0 ||
      !n_pairs || (capacity > 0 && !pairs))
    return OKVIS_BA_ERR_ARG;
  *n_pairs = 0;
  if (n_a == 0 || n_b == 0) return OKVIS_BA_OK;
  if (!desc_a || !desc_b) return OKVIS_BA_ERR_ARG;
  FE_TRY(hipSetDevice(c->device));
  const size_t na = (size_t)n_a, nb = (size_t)n_b, cap = (size_t)capacity, db = (size_t)desc_bytes;
  Stage st{c};
  const auto s_da = st.in<uint8_t>(db * na), s_db = st.in<uint8_t>(db * nb);
  const auto s_sa = st.in<uint8_t>(na, skip_a != nullptr), s_sb = st.in<uint8_t>(nb, skip_b != nullptr);
  const auto s_cnt = st.scratch<int32_t>(na);
  const auto s_off = st.scratch<unsigned long long>(na);
  const auto s_tot = st.out<unsigned long long>(1);  // back: from the total onward
  const auto s_pairs = st.out<int32_t>(2 * cap);
  const auto s_dist = st.out<float>(cap);
  if (int rc = st.reserve()) return rc;
  st.put(s_da, desc_a), st.put(s_db, desc_b), st.put(s_sa, skip_a), st.put(s_sb, skip_b);
  if (int rc = st.upload()) return rc;
  fe::CandParams P;
  P.desc_a = st.dev(s_da), P.desc_b = st.dev(s_db), P.skip_a = st.dev(s_sa), P.skip_b = st.dev(s_sb);
  P.n_a = n_a, P.n_b = n_b, P.threshold = threshold;
  P.counts = st.dev(s_cnt), P.offsets = st.dev(s_off);
  P.capacity = capacity, P.pairs = st.dev(s_pairs), P.dist = st.dev(s_dist);
  launch_hamming_rows<false>(desc_bytes / 16, P, c->stream);
  FE_TRY(hipGetLastError());
  hipLaunchKernelGGL(fe::row_offsets_kernel, dim3(1), dim3(fe::SCAN_THREADS), 0, c->stream, (const int32_t*)P.counts, st.dev(s_off),
                     st.dev(s_tot), n_a);
  FE_TRY(hipGetLastError());
  if (capacity > 0) {
    launch_hamming_rows<true>(desc_bytes / 16, P, c->stream);
    FE_TRY(hipGetLastError());
  }
  if (int rc = st.download()) return rc;
  const unsigned long long total = *st.host(s_tot);
  *n_pairs = total > (unsigned long long)INT32_MAX ? INT32_MAX : (int32_t)total;
  const size_t n = total < cap ? (size_t)total : cap;  // of the capacity, the pairs there are
  if (n) std::copy_n(st.host(s_pairs), 2 * n, pairs);
  if (n && dist) std::copy_n(st.host(s_dist), n, dist);
  return OKVIS_BA_OK;
}

int okvis_fe_match_descriptors(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_match_job* jobs, int32_t desc_bytes, float threshold,
                               int32_t num_best, int32_t use_ratio, float ratio_threshold) {
  if (!match_call_ok(c, n_jobs, jobs, desc_bytes, num_best, use_ratio)) return OKVIS_BA_ERR_ARG;
  size_t rows = 0, blocks = 0, n_live = 0;  // n_live: jobs with keypoints on both sides; the others yield nothing
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_match_job& J = jobs[j];
    if (!match_job_ok(J)) return OKVIS_BA_ERR_ARG;
    if (J.n_a > 0 && J.n_b > 0) ++n_live, rows += (size_t)J.n_a, blocks += match_blocks(J.n_a);
  }
  if (blocks > (size_t)INT32_MAX || rows > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
  const size_t db = (size_t)desc_bytes, nbest = (size_t)num_best;
  Stage st{c};
  Staged<int32_t> s_lidx;
  Staged<float> s_ldist;
  if (rows > 0) {
    FE_TRY(hipSetDevice(c->device));
    // every job's descriptors and masks, then the job table
    struct Plan {
      Staged<uint8_t> da, db, sa, sb;
    };
    std::vector<Plan> plan((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_match_job& J = jobs[j];
      if (J.n_a == 0 || J.n_b == 0) continue;
      Plan& p = plan[j];
      p.da = st.in<uint8_t>(db * J.n_a), p.db = st.in<uint8_t>(db * J.n_b);
      p.sa = st.in<uint8_t>((size_t)J.n_a, J.skip_a != nullptr), p.sb = st.in<uint8_t>((size_t)J.n_b, J.skip_b != nullptr);
    }
    const auto s_table = st.in<fe::MatchJob>(n_live);
    s_lidx = st.out<int32_t>(rows * nbest), s_ldist = st.out<float>(rows * nbest);
    if (int rc = st.reserve()) return rc;
    fe::MatchJob* table = st.host(s_table);
    int32_t block0 = 0, row0 = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_match_job& J = jobs[j];
      if (J.n_a == 0 || J.n_b == 0) continue;
      const Plan& p = plan[j];
      st.put(p.da, J.desc_a), st.put(p.db, J.desc_b), st.put(p.sa, J.skip_a), st.put(p.sb, J.skip_b);
      fe::MatchJob D;
      D.desc_a = st.dev(p.da), D.desc_b = st.dev(p.db), D.skip_a = st.dev(p.sa), D.skip_b = st.dev(p.sb);
      D.n_a = J.n_a, D.n_b = J.n_b, D.block0 = block0, D.row0 = row0;
      *table++ = D;
      block0 += (int32_t)match_blocks(J.n_a), row0 += J.n_a;
    }
    if (int rc = st.upload()) return rc;
    fe::BestParams P;
    P.jobs = st.dev(s_table), P.n_jobs = (int32_t)n_live;
    fill_list_params(P, st, threshold, num_best, use_ratio, s_lidx, s_ldist);
    with_words(desc_bytes / 16, [&](auto w) {
      hipLaunchKernelGGL(fe::best_lists_kernel<w()>, dim3((unsigned)blocks), dim3(fe::MATCH_THREADS), 0, c->stream, P);
    });
    FE_TRY(hipGetLastError());
    if (int rc = st.download()) return rc;
  }
  size_t row0 = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_match_job& J = jobs[j];
    assign_and_accept(J, st.host(s_lidx) + row0 * nbest, st.host(s_ldist) + row0 * nbest, num_best, threshold, use_ratio, ratio_threshold,
                      [](int, size_t) {});
    if (J.n_a > 0 && J.n_b > 0) row0 += (size_t)J.n_a;
  }
  return OKVIS_BA_OK;
}

int okvis_fe_match_verified(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_vmatch_job* jobs, int32_t desc_bytes, float threshold,
                            int32_t num_best, int32_t use_ratio, float ratio_threshold) {
  if (!match_call_ok(c, n_jobs, jobs, desc_bytes, num_best, use_ratio)) return OKVIS_BA_ERR_ARG;
  // per job: live = keypoints on both sides (lists are built); pre = the per-keypoint pass has something to do (a 3D2D step
  // reports its projections even against an empty image B); tri = the accepted pairs' uncertainty is wanted
  struct Plan {
    bool live, pre, tri;
    Staged<uint8_t> da, db, sa, sb;       // in
    Staged<float> ka, kb;
    Staged<double> hp, sga, sgb;
    Staged<double> ra, rb;                // device only: the rays
    Staged<double> uv, U;                 // back
    Staged<uint8_t> st;
    Staged<int32_t> t_pairs;              // the uncertainty launch takes ...
    Staged<double> t_sig;
    Staged<double> t_hp, t_cov;           // ... and gives
    Staged<uint8_t> t_fl;
    double info6[36];
  };
  std::vector<Plan> plan((size_t)n_jobs);
  size_t rows = 0, blocks = 0, pre_blocks = 0, n_work = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_vmatch_job& J = jobs[j];
    Plan& p = plan[j];
    const bool is2d = J.kind == OKVIS_FE_MATCH_2D2D;
    if ((!is2d && J.kind != OKVIS_FE_MATCH_3D2D) || !match_job_ok(J) || !camera_ok(&J.cam_a) || !camera_ok(&J.cam_b)) return OKVIS_BA_ERR_ARG;
    if (!J.kp_b || (is2d && !J.kp_a) || (!is2d && J.n_a > 0 && !J.hp_W)) return OKVIS_BA_ERR_ARG;
    p.live = J.n_a > 0 && J.n_b > 0;
    p.pre = is2d ? p.live : J.n_a > 0;
    p.tri = is2d && (J.hp_a || J.cov || J.tri_flags);
    if (p.tri && !spd_inverse6(J.UOplus, p.info6)) return OKVIS_BA_ERR_ARG;
    p.tri = p.tri && p.live;
    if (p.live) rows += (size_t)J.n_a, blocks += match_blocks(J.n_a);
    if (p.pre) ++n_work, pre_blocks += prepass_blocks(J);
  }
  if (blocks > (size_t)INT32_MAX || rows > (size_t)INT32_MAX || pre_blocks > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
  const size_t db = (size_t)desc_bytes, nbest = (size_t)num_best;
  Stage st{c};
  Staged<int32_t> s_lidx;
  Staged<float> s_ldist;
  Staged<double> s_lchi;
  Staged<uint8_t> s_lfl;
  if (n_work > 0) {
    FE_TRY(hipSetDevice(c->device));
    // in: every job's descriptors, masks, keypoints, landmarks and ray sigmas, then the job table; device only: the rays;
    // back: the projections and the lists; then what the uncertainty launches take and give
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_vmatch_job& J = jobs[j];
      Plan& p = plan[j];
      if (!p.pre) continue;
      const bool is2d = J.kind == OKVIS_FE_MATCH_2D2D;
      const size_t na = (size_t)J.n_a, nb = (size_t)J.n_b;
      p.da = st.in<uint8_t>(db * na, p.live), p.db = st.in<uint8_t>(db * nb, p.live), p.kb = st.in<float>(3 * nb, p.live);
      p.sa = st.in<uint8_t>(na, J.skip_a != nullptr), p.sb = st.in<uint8_t>(nb, p.live && J.skip_b);
      p.ka = st.in<float>(3 * na, is2d), p.sga = st.in<double>(na, is2d), p.sgb = st.in<double>(nb, is2d);
      p.hp = st.in<double>(4 * na, !is2d);
    }
    const auto s_table = st.in<fe::VJob>(n_work);
    for (int j = 0; j < n_jobs; ++j) {
      const bool rays = plan[j].pre && jobs[j].kind == OKVIS_FE_MATCH_2D2D;
      plan[j].ra = st.scratch<double>(3 * (size_t)jobs[j].n_a, rays), plan[j].rb = st.scratch<double>(3 * (size_t)jobs[j].n_b, rays);
    }
    for (int j = 0; j < n_jobs; ++j) {
      const bool proj = plan[j].pre && jobs[j].kind == OKVIS_FE_MATCH_3D2D;
      const size_t na = (size_t)jobs[j].n_a;
      plan[j].uv = st.out<double>(2 * na, proj), plan[j].U = st.out<double>(4 * na, proj), plan[j].st = st.out<uint8_t>(na, proj);
    }
    s_lidx = st.out<int32_t>(rows * nbest), s_ldist = st.out<float>(rows * nbest);
    s_lchi = st.out<double>(rows * nbest), s_lfl = st.out<uint8_t>(rows * nbest);
    for (int j = 0; j < n_jobs; ++j) {
      const size_t nb = (size_t)jobs[j].n_b;
      plan[j].t_pairs = st.scratch<int32_t>(2 * nb, plan[j].tri), plan[j].t_sig = st.scratch<double>(nb, plan[j].tri);
    }
    for (int j = 0; j < n_jobs; ++j) {
      const size_t nb = (size_t)jobs[j].n_b;
      Plan& p = plan[j];
      p.t_hp = st.scratch<double>(4 * nb, p.tri), p.t_cov = st.scratch<double>(9 * nb, p.tri), p.t_fl = st.scratch<uint8_t>(nb, p.tri);
    }
    if (int rc = st.reserve()) return rc;
    fe::VJob* table = st.host(s_table);
    int32_t block0 = 0, row0 = 0, pre0 = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_vmatch_job& J = jobs[j];
      const Plan& p = plan[j];
      if (!p.pre) continue;
      const bool is2d = J.kind == OKVIS_FE_MATCH_2D2D;
      const size_t na = (size_t)J.n_a, nb = (size_t)J.n_b;
      st.put(p.da, J.desc_a), st.put(p.db, J.desc_b), st.put(p.kb, J.kp_b), st.put(p.sa, J.skip_a), st.put(p.sb, J.skip_b);
      st.put(p.ka, J.kp_a), st.put(p.hp, J.hp_W);
      fe::VJob D;
      std::memset(&D, 0, sizeof(D));
      D.desc_a = st.dev(p.da), D.desc_b = st.dev(p.db), D.kp_b = st.dev(p.kb), D.skip_a = st.dev(p.sa), D.skip_b = st.dev(p.sb);
      D.kp_a = st.dev(p.ka), D.sig_a = st.dev(p.sga), D.sig_b = st.dev(p.sgb), D.ray_a = st.dev(p.ra), D.ray_b = st.dev(p.rb);
      D.hp_W = st.dev(p.hp), D.uv = st.dev(p.uv), D.U = st.dev(p.U), D.status = st.dev(p.st);
      if (is2d) {
        double *sga = st.host(p.sga), *sgb = st.host(p.sgb);
        for (size_t k = 0; k < na; ++k) sga[k] = ray_sigma(J.kp_a[3 * k + 2], J.cam_a.intr[0]);
        for (size_t k = 0; k < nb; ++k) sgb[k] = ray_sigma(J.kp_b[3 * k + 2], J.cam_b.intr[0]);
        std::memcpy(D.T, J.T_AB, sizeof(D.T));
      } else {
        std::memcpy(D.T, J.T_CbW, sizeof(D.T));
        std::memcpy(D.P3, J.P3, sizeof(D.P3));
      }
      D.cam_a = to_device(&J.cam_a), D.cam_b = to_device(&J.cam_b);
      D.kind = J.kind, D.n_a = J.n_a, D.n_b = J.n_b, D.block0 = block0, D.row0 = row0, D.pre0 = pre0;
      *table++ = D;
      if (p.live) block0 += (int32_t)match_blocks(J.n_a), row0 += J.n_a;
      pre0 += (int32_t)prepass_blocks(J);
    }
    if (int rc = st.upload()) return rc;
    hipLaunchKernelGGL(fe::vmatch_prepass_kernel, dim3((unsigned)pre_blocks), dim3(fe::VMATCH_PRE_THREADS), 0, c->stream,
                       (const fe::VJob*)st.dev(s_table), (int)n_work);
    FE_TRY(hipGetLastError());
    if (blocks > 0) {
      fe::VListParams P;
      P.jobs = st.dev(s_table), P.n_jobs = (int32_t)n_work;
      fill_list_params(P, st, threshold, num_best, use_ratio, s_lidx, s_ldist);
      P.list_chi2 = st.dev(s_lchi), P.list_flags = st.dev(s_lfl);
      with_words(desc_bytes / 16, [&](auto w) {
        hipLaunchKernelGGL(fe::verified_lists_kernel<w()>, dim3((unsigned)blocks), dim3(fe::MATCH_THREADS), 0, c->stream, P);
      });
      FE_TRY(hipGetLastError());
    }
    if (int rc = st.download()) return rc;
  }
  // the assignment chains and matchBody's final loop on the host, as okvis_fe_match_descriptors; then what setBestMatch computes
  // again for the accepted pairs: 3D2D from the list entry, 2D2D through one launch of stereo_triangulate_kernel per job
  size_t row0 = 0, tri_lo = SIZE_MAX, tri_hi = 0, tri_out_lo = SIZE_MAX, tri_out_hi = 0;
  std::vector<int32_t> n_acc((size_t)n_jobs, 0);
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_vmatch_job& J = jobs[j];
    const Plan& p = plan[j];
    const bool is2d = J.kind == OKVIS_FE_MATCH_2D2D;
    const size_t na = (size_t)J.n_a, nb = (size_t)J.n_b;
    const auto zero = [](auto* dst, size_t n) { if (dst) std::fill_n(dst, n, 0); };
    zero(J.chi2, nb), zero(J.gate_flags, nb), zero(J.hp_a, 4 * nb), zero(J.cov, 9 * nb), zero(J.tri_flags, nb);
    if (p.st.on) st.get(p.st, J.proj_status), st.get(p.uv, J.uv), st.get(p.U, J.U);
    else zero(J.proj_status, na), zero(J.uv, 2 * na), zero(J.U, 4 * na);
    const int32_t* li = st.host(s_lidx) + row0 * nbest;
    const float* ld = st.host(s_ldist) + row0 * nbest;
    const double* lc = st.host(s_lchi) + row0 * nbest;
    const uint8_t* lf = st.host(s_lfl) + row0 * nbest;
    int32_t* t_pairs = st.host(p.t_pairs);
    double* t_sig = st.host(p.t_sig);
    assign_and_accept(J, li, ld, num_best, threshold, use_ratio, ratio_threshold, [&](int b, size_t o) {
      if (!is2d) {
        for (size_t k = 0; k < nbest; ++k)
          if (li[o + k] == b) {
            if (J.chi2) J.chi2[b] = lc[o + k];
            if (J.gate_flags) J.gate_flags[b] = lf[o + k];
            break;
          }
      } else if (p.tri) {
        const int32_t a = J.pair_a[b], i = n_acc[j]++;
        t_pairs[2 * i] = a, t_pairs[2 * i + 1] = b;
        t_sig[i] = std::fmax(ray_sigma(J.kp_a[3 * a + 2], J.cam_a.intr[0]), ray_sigma(J.kp_b[3 * b + 2], J.cam_b.intr[0]));
      }
    });
    if (p.live) row0 += na;
    if (n_acc[j] > 0) {
      tri_lo = std::min(tri_lo, p.t_pairs.off), tri_hi = std::max(tri_hi, p.t_sig.end());
      tri_out_lo = std::min(tri_out_lo, p.t_hp.off), tri_out_hi = std::max(tri_out_hi, p.t_fl.end());
    }
  }
  if (tri_hi > 0) {
    // by hand: a second copy in and a second copy back, over the jobs that accepted something
    FE_TRY(hipMemcpyAsync(c->d_stage + tri_lo, c->h_stage + tri_lo, tri_hi - tri_lo, hipMemcpyHostToDevice, c->stream));
    for (int j = 0; j < n_jobs; ++j) {
      if (n_acc[j] == 0) continue;
      const okvis_fe_vmatch_job& J = jobs[j];
      const Plan& p = plan[j];
      fe::TriParams P;
      std::memcpy(P.info6, p.info6, sizeof(P.info6));
      P.n_a = J.n_a, P.n_b = J.n_b, P.n_pairs = n_acc[j], P.want_uncertainty = 1;
      P.kp_a = st.dev(p.ka), P.kp_b = st.dev(p.kb), P.pairs = st.dev(p.t_pairs), P.sigma_ray = st.dev(p.t_sig);
      P.hp = st.dev(p.t_hp), P.cov = st.dev(p.t_cov), P.flags = st.dev(p.t_fl), P.gn = nullptr;
      if (int rc = launch_triangulate(c, P, &J.cam_a, &J.cam_b, J.T_AB, true)) return rc;
    }
    FE_TRY(hipMemcpyAsync(c->h_stage + tri_out_lo, c->d_stage + tri_out_lo, tri_out_hi - tri_out_lo, hipMemcpyDeviceToHost, c->stream));
    FE_TRY(hipStreamSynchronize(c->stream));
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_vmatch_job& J = jobs[j];
      const Plan& p = plan[j];
      const int32_t* t_pairs = st.host(p.t_pairs);
      for (int i = 0; i < n_acc[j]; ++i) {
        const size_t b = (size_t)t_pairs[2 * i + 1];
        if (J.hp_a) std::copy_n(st.host(p.t_hp) + 4 * i, 4, J.hp_a + 4 * b);
        if (J.cov) std::copy_n(st.host(p.t_cov) + 9 * i, 9, J.cov + 9 * b);
        if (J.tri_flags) J.tri_flags[b] = st.host(p.t_fl)[i];
      }
    }
  }
  return OKVIS_BA_OK;
}

}  // extern "C"
