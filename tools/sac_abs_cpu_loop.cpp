// The work of okvis_fe_sac_solve_absolute's solver launch as a loop on one CPU core, with the core the kernel runs
// (okvis_amd/csrc/fe_sac_gp3p.hpp; gp3_group called with lane 0, stride 1).  For scale next to the GPU timing in
// scripts/bench_sac_abs.py.  Not part of the library: the product has no CPU path.
//   g++ -O2 -std=c++17 -shared -fPIC tools/sac_abs_cpu_loop.cpp -o sac_abs_cpu_loop.so
#include <algorithm>
#include <vector>

#include "../okvis_amd/csrc/fe_sac_gp3p.hpp"

extern "C" {

// one job: the inputs as okvis_fe_sac_absolute_job has them; models [n_models][12], valid [n_models]
int sac_abs_cpu_job(const okvis_fe_sac_absolute_job* J, double* models, uint8_t* valid) {
  const size_t n = (size_t)J->n;
  std::vector<double> a(3 * n), b(3 * n), cams(12 * (size_t)J->n_cams), slab(fe::GP3_SLAB);
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) a[k * n + i] = J->points[3 * i + k], b[k * n + i] = J->bearing[3 * i + k];
  for (int k = 0; k < J->n_cams; ++k) {
    std::copy_n(J->cam_offsets + 3 * k, 3, cams.data() + 12 * k);
    std::copy_n(J->cam_rotations + 9 * k, 9, cams.data() + 12 * k + 3);
  }
  for (int m = 0; m < J->n_models; ++m) {
    fe::Gp3Out out;
    out.model = models + 12 * (size_t)m, out.valid = valid + m, out.n_roots = nullptr, out.candidates = nullptr;
    fe::gp3_group(slab.data(), 0, 1, a.data(), b.data(), n, J->cam_index, cams.data(), J->samples + 4 * (size_t)m, out);
  }
  return 0;
}

int sac_abs_cpu(int32_t n_jobs, const okvis_fe_sac_absolute_job* jobs) {
  for (int j = 0; j < n_jobs; ++j) sac_abs_cpu_job(jobs + j, jobs[j].models, jobs[j].valid);
  return 0;
}
}
