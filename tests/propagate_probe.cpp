// TEST INFRASTRUCTURE.  The step functions of okvis_amd/csrc/fe_propagate.hpp (BA_HD: a plain host compiler sees them) driven on
// the CPU the way imu_propagate_kernel drives them, lane by lane: the serial walk over the deque, F_delta applied to the columns of
// P_delta, the transposition, F_delta applied to the rows.  tests/test_imu_propagate_host.py compiles this file with
// -ffp-contract=off and holds it against the long double referee, so that the device arithmetic is judged without a GPU; the
// kernel's own control flow (the ballot scan, the LDS window) is what tests/test_gpu_imu_propagate.py is for.
#include <cstring>

#include "../okvis_amd/csrc/fe_propagate.hpp"

extern "C" int probe_imu_propagation(int n, const int64_t* ts, const double* gyr, const double* acc, const okvis_ba_imu_params* prm,
                                     double* T, double* sb, int64_t t_start, int64_t t_end, double* cov, double* jac) {
  using namespace fe;
  if (n < 2) return 0;
  if (!(ts[n - 1] >= t_end)) return -1;
  PropState S;
  PropF F;
  prop_reset(&S);
  double P[15][15] = {{0}}, M[15][15];
  long long time = t_start;
  bool started = false;
  int i = 0;
  for (int it = 0; it < n; ++it) {
    const int nx = it + 1 < n ? it + 1 : it;
    double w0[3], a0[3], w1[3], a1[3];
    for (int c = 0; c < 3; ++c) w0[c] = gyr[3 * it + c], a0[c] = acc[3 * it + c], w1[c] = gyr[3 * nx + c], a1[c] = acc[3 * nx + c];
    long long nexttime = it + 1 == n ? t_end : ts[it + 1];
    double dt = prop_sec(nexttime - time);
    if (t_end < nexttime) {
      const double interval = prop_sec(nexttime - ts[it]);
      nexttime = t_end;
      dt = prop_sec(nexttime - time);
      const double r = dt / interval;
      for (int c = 0; c < 3; ++c) w1[c] = (1.0 - r) * w0[c] + r * w1[c], a1[c] = (1.0 - r) * a0[c] + r * a1[c];
    }
    if (dt <= 0.0) continue;
    if (!started) {
      started = true;
      const double r = dt / prop_sec(nexttime - ts[it]);
      for (int c = 0; c < 3; ++c) w0[c] = r * w0[c] + (1.0 - r) * w1[c], a0[c] = r * a0[c] + (1.0 - r) * a1[c];
    }
    prop_step(*prm, w0, a0, w1, a1, dt, sb, &S, cov != nullptr, &F, true);
    if (cov) {
      for (int lane = 0; lane < 15; ++lane) {  // column `lane` of F P
        double x[15], y[15];
        for (int k = 0; k < 15; ++k) x[k] = P[k][lane];
        prop_apply(F, x, y);
        for (int k = 0; k < 15; ++k) M[k][lane] = y[k];
      }
      for (int lane = 0; lane < 15; ++lane) {  // row `lane` of (F P) F^T, plus the noise
        double y[15];
        prop_apply(F, M[lane], y);
        for (int k = 0; k < 15; ++k) P[lane][k] = k == lane ? y[k] + prop_noise(F, k) : y[k];
      }
    }
    time = nexttime;
    ++i;
    if (nexttime == t_end) break;
  }
  double C0[9];
  prop_finish(*prm, S, T, sb, C0, jac != nullptr, &F, true);
  if (jac)
    for (int lane = 0; lane < 15; ++lane) {
      double x[15], y[15];
      for (int k = 0; k < 15; ++k) x[k] = k == lane ? 1.0 : 0.0;
      prop_apply(F, x, y);
      for (int k = 0; k < 15; ++k) jac[15 * k + lane] = y[k];
    }
  if (cov) {
    for (int lane = 0; lane < 15; ++lane) {
      double x[15], y[15];
      for (int k = 0; k < 15; ++k) x[k] = P[k][lane];
      prop_rotate(C0, x, y);
      for (int k = 0; k < 15; ++k) M[k][lane] = y[k];
    }
    for (int lane = 0; lane < 15; ++lane) prop_rotate(C0, M[lane], cov + 15 * lane);
  }
  return i;
}
