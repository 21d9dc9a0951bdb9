// The host side of okvis_amd/csrc/fe_sac_gp3p.hpp as a stand-alone program: the same gp3_group the kernel runs, called with
// (lane 0, stride 1) so that every "lanes take ..." loop runs in order.  tests/test_sac_abs_host.py builds it with
// -fsanitize=address,undefined and holds it to the device's bounds.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/sac_abs_probe.cpp -o sac_abs_probe
//   sac_abs_probe IN OUT
// IN  (raw, little endian): int32 n, n_cams, k, 0; double points[n][3], bearing[n][3]; int32 cam_index[n]; double
//     cam_offsets[n_cams][3], cam_rotations[n_cams][9]; int32 samples[k][4]
// OUT (raw): per sample 110 doubles: valid, n_roots, model[12], candidates[8][12] (NaN past n_roots)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../okvis_amd/csrc/fe_sac_gp3p.hpp"

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
  const int n = head[0], n_cams = head[1], k = head[2];
  if (n < 0 || n_cams < 1 || n_cams > 8 || k < 0) return 2;
  std::vector<double> pts(3 * (size_t)n), brg(3 * (size_t)n), off(3 * (size_t)n_cams), rot(9 * (size_t)n_cams);
  std::vector<int32_t> ci((size_t)n), q(4 * (size_t)k);
  if (!read_all(in, pts) || !read_all(in, brg) || !read_all(in, ci) || !read_all(in, off) || !read_all(in, rot) || !read_all(in, q)) return 2;
  fclose(in);
  for (int32_t i : q)
    if (i < 0 || i >= n) return 3;
  for (int32_t i : ci)
    if (i < 0 || i >= n_cams) return 3;
  // the device layout: [3][n], cams [n_cams][12]
  std::vector<double> a(3 * (size_t)n), b(3 * (size_t)n), cams(12 * (size_t)n_cams);
  for (int i = 0; i < n; ++i)
    for (int e = 0; e < 3; ++e) a[(size_t)e * n + i] = pts[3 * (size_t)i + e], b[(size_t)e * n + i] = brg[3 * (size_t)i + e];
  for (int c = 0; c < n_cams; ++c) {
    for (int e = 0; e < 3; ++e) cams[12 * (size_t)c + e] = off[3 * (size_t)c + e];
    for (int e = 0; e < 9; ++e) cams[12 * (size_t)c + 3 + e] = rot[9 * (size_t)c + e];
  }
  std::vector<double> out(110 * (size_t)k, fe::sac_nan());
  std::vector<double> slab(fe::GP3_SLAB, 0.0);
  for (int m = 0; m < k; ++m) {
    double* o = out.data() + 110 * (size_t)m;
    uint8_t valid = 0;
    int32_t roots = 0;
    fe::Gp3Out dst;
    dst.model = o + 2, dst.valid = &valid, dst.n_roots = &roots, dst.candidates = o + 14;
    fe::gp3_group(slab.data(), 0, 1, a.data(), b.data(), (size_t)n, ci.data(), cams.data(), q.data() + 4 * (size_t)m, dst);
    o[0] = valid, o[1] = roots;
  }
  FILE* f = fopen(argv[2], "wb");
  if (!f) return 2;
  const bool wrote = out.empty() || fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  return fclose(f) == 0 && wrote ? 0 : 2;
}
