// The host side of okvis_amd/csrc/fe_sac_solve.hpp as a stand-alone program: the same BA_HD building blocks and the same
// sac5_wave the kernel runs, called with (lane 0, stride 1) so that every "lanes take ..." loop runs in order.
// tests/test_sac_solve_host.py builds it with -fsanitize=address,undefined and holds it to the device's bounds.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/sac_solve_probe.cpp -o sac_solve_probe
//   sac_solve_probe IN OUT
// IN  (raw, little endian): int32 n, n5, n2, has_sigma; double bearing1[n][3], bearing2[n][3], sigma1[n], sigma2[n] (the sigmas
//     only with has_sigma); int32 samples5[n5][8], samples2[n2][2]
// OUT (raw): per five-point sample 104 doubles: valid, n_roots, model[12], essentials[10][9] (NaN past n_roots);
//     then per two-point sample 10 doubles: valid, R[9]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../okvis_amd/csrc/fe_sac_solve.hpp"

template <class T>
static bool read_all(FILE* f, std::vector<T>& v) {
  return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t head[4];
  if (fread(head, sizeof(int32_t), 4, in) != 4) return 2;
  const int n = head[0], n5 = head[1], n2 = head[2];
  const bool has_sigma = head[3] != 0;
  if (n < 0 || n5 < 0 || n2 < 0) return 2;
  std::vector<double> b1(3 * (size_t)n), b2(3 * (size_t)n), s1(has_sigma ? n : 0), s2(has_sigma ? n : 0);
  std::vector<int32_t> q5(8 * (size_t)n5), q2(2 * (size_t)n2);
  if (!read_all(in, b1) || !read_all(in, b2) || !read_all(in, s1) || !read_all(in, s2) || !read_all(in, q5) || !read_all(in, q2)) return 2;
  fclose(in);
  for (int32_t i : q5)
    if (i < 0 || i >= n) return 3;
  for (int32_t i : q2)
    if (i < 0 || i >= n) return 3;
  // the device layout: [3][n]
  std::vector<double> a(3 * (size_t)n), b(3 * (size_t)n);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) a[(size_t)k * n + i] = b1[3 * (size_t)i + k], b[(size_t)k * n + i] = b2[3 * (size_t)i + k];
  std::vector<double> out(104 * (size_t)n5 + 10 * (size_t)n2, fe::sac_nan());
  std::vector<double> slab(fe::SOLVE_SLAB, 0.0);
  for (int m = 0; m < n5; ++m) {
    double* o = out.data() + 104 * (size_t)m;
    uint8_t valid = 0;
    int32_t roots = 0;
    fe::Sac5Out dst;
    dst.model = o + 2, dst.valid = &valid, dst.n_roots = &roots, dst.essentials = o + 14;
    fe::sac5_wave(slab.data(), 0, 1, a.data(), b.data(), (size_t)n, has_sigma ? s1.data() : nullptr, has_sigma ? s2.data() : nullptr,
                  q5.data() + 8 * (size_t)m, dst);
    o[0] = valid, o[1] = roots;
  }
  for (int m = 0; m < n2; ++m) {
    double* o = out.data() + 104 * (size_t)n5 + 10 * (size_t)m;
    const int32_t i = q2[2 * (size_t)m], j = q2[2 * (size_t)m + 1];
    double R[9];
    const bool ok = i != j && fe::sac2_rotation(&b1[3 * (size_t)i], &b1[3 * (size_t)j], &b2[3 * (size_t)i], &b2[3 * (size_t)j], R);
    o[0] = ok ? 1.0 : 0.0;
    for (int e = 0; e < 9; ++e) o[1 + e] = ok ? R[e] : fe::sac_nan();
  }
  FILE* f = fopen(argv[2], "wb");
  if (!f) return 2;
  const bool wrote = out.empty() || fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  return fclose(f) == 0 && wrote ? 0 : 2;
}
