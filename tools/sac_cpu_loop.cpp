// The work of okvis_fe_sac_consensus as a loop on one CPU core, with the score functions the kernel uses
// (okvis_amd/csrc/fe_sac.hpp; they are host-compilable).  For scale next to the GPU timing in tools/time_sac_consensus.py, and a
// way to look at the formulas' results without a GPU.  Not part of the library: the product has no CPU path.
//   g++ -O2 -std=c++17 -shared -fPIC tools/sac_cpu_loop.cpp -o sac_cpu_loop.so
#include <cstring>

#include "../okvis_amd/csrc/fe_sac.hpp"

extern "C" {

// one job: counts [n_models] always, scores [n_models][n] if not null.  a / b: [n][3] as okvis_fe_sac_job has them.
int sac_cpu_job(const okvis_fe_sac_job* J, int32_t* counts, double* scores) {
  double h[fe::SAC_MODEL_STRIDE] = {0};
  const bool absolute = J->kind == OKVIS_FE_SAC_ABSOLUTE;
  const double *a = absolute ? J->points : J->bearing1, *b = absolute ? J->bearing : J->bearing2;
  const double* s1 = absolute ? J->sigma : J->sigma1;
  for (int m = 0; m < J->n_models; ++m) {
    fe::sac_stage_model(J->kind, J->models + (size_t)m * (J->kind == OKVIS_FE_SAC_ROTATION_ONLY ? 9 : 12), h);
    int32_t count = 0;
    for (int i = 0; i < J->n; ++i) {
      double s;
      if (absolute) {
        double cam[12];
        std::memcpy(cam, J->cam_offsets + 3 * J->cam_index[i], sizeof(double) * 3);
        std::memcpy(cam + 3, J->cam_rotations + 9 * J->cam_index[i], sizeof(double) * 9);
        s = fe::sac_score_absolute(h, a + 3 * i, b + 3 * i, s1[i], cam);
      } else if (J->kind == OKVIS_FE_SAC_ROTATION_ONLY) {
        s = fe::sac_score_rotation_only(h, a + 3 * i, b + 3 * i, s1[i], J->sigma2[i]);
      } else {
        s = fe::sac_score_relative(h, a + 3 * i, b + 3 * i, s1[i], J->sigma2[i]);
      }
      count += s < J->threshold ? 1 : 0;
      if (scores) scores[(size_t)m * J->n + i] = s;
    }
    counts[m] = count;
  }
  return 0;
}

int sac_cpu_consensus(int32_t n_jobs, const okvis_fe_sac_job* jobs) {
  for (int j = 0; j < n_jobs; ++j)
    if (jobs[j].counts) sac_cpu_job(jobs + j, jobs[j].counts, jobs[j].scores);
  return 0;
}
}
