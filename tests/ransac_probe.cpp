// The host side of okvis_amd/csrc/fe_sac_loop.hpp as a stand-alone program: the same BA_HD generator, draw, decision function and
// sequential rule the kernels are built from.  tests/test_ransac_host.py builds it with -fsanitize=address,undefined and holds it to
// tests/ransac_statement.py exactly.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/ransac_probe.cpp -o ransac_probe
//   ransac_probe IN OUT
// IN  (raw, little endian): int32 n_philox, n_sample, n_loop, n_done; then
//     n_philox x { uint32 counter[4], key[2] }
//     n_sample x { uint64 seed; int32 n, n_slots, s, 0 }
//     n_loop   x { int32 n, n_slots, s, max_iterations; double p; int32 counts[n_slots]; int32 valid[n_slots] }
//     n_done   x { int32 it, c, n, s; double p }
// OUT (raw): int32 / uint32 words in the same order: 4 per Philox block, n_slots * s per sample case, 5 per loop case (best,
//     n_inliers, iterations, skipped, stop), 1 per decision
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../okvis_amd/csrc/fe_sac_loop.hpp"

template <class T>
static bool get(FILE* f, T* v, size_t n = 1) {
  return n == 0 || fread(v, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t head[4];
  if (!get(in, head, 4)) return 2;
  for (int32_t h : head)
    if (h < 0) return 2;
  std::vector<int32_t> out;
  for (int i = 0; i < head[0]; ++i) {
    uint32_t w[6], u[4];
    if (!get(in, w, 6)) return 2;
    fe::sac_philox(w[0], w[1], w[2], w[3], w[4], w[5], u);
    for (uint32_t x : u) out.push_back((int32_t)x);
  }
  for (int i = 0; i < head[1]; ++i) {
    uint64_t seed;
    int32_t a[4];
    if (!get(in, &seed) || !get(in, a, 4)) return 2;
    const int n = a[0], n_slots = a[1], s = a[2];
    if (s < 1 || s > fe::SAC_MAX_SAMPLE || n < s || n_slots < 0) return 3;
    for (int m = 0; m < n_slots; ++m) {
      std::vector<int32_t> q((size_t)s, -1);  // exactly s entries: the sanitizer sees a write past them
      fe::sac_draw_sample(seed, (uint32_t)m, (uint32_t)n, s, q.data());
      out.insert(out.end(), q.begin(), q.end());
    }
  }
  for (int i = 0; i < head[2]; ++i) {
    int32_t a[4];
    double p;
    if (!get(in, a, 4) || !get(in, &p)) return 2;
    const int n = a[0], n_slots = a[1], s = a[2], max_iterations = a[3];
    if (n < 1 || n_slots < 0 || s < 1 || max_iterations < 1) return 3;
    std::vector<int32_t> counts((size_t)n_slots), valid32((size_t)n_slots);
    if (!get(in, counts.data(), counts.size()) || !get(in, valid32.data(), valid32.size())) return 2;
    std::vector<uint8_t> valid(valid32.begin(), valid32.end());
    const fe::SacLoopState L = fe::sac_loop_rule(counts.data(), valid.data(), n_slots, n, s, max_iterations, p);
    out.push_back(L.best), out.push_back(L.best >= 0 ? L.best_count : 0), out.push_back(L.iterations), out.push_back(L.skipped);
    out.push_back(L.stop);
  }
  for (int i = 0; i < head[3]; ++i) {
    int32_t a[4];
    double p;
    if (!get(in, a, 4) || !get(in, &p)) return 2;
    out.push_back(fe::sac_done(a[0], a[1], a[2], a[3], p) ? 1 : 0);
  }
  fclose(in);
  FILE* f = fopen(argv[2], "wb");
  if (!f) return 2;
  const bool wrote = out.empty() || fwrite(out.data(), sizeof(int32_t), out.size(), f) == out.size();
  return fclose(f) == 0 && wrote ? 0 : 2;
}
