// The host's candidate search as BatchedKeyframeWindowMatching::doSetup ran it before okvis_fe_hamming_candidates (and still runs it
// with deviceCandidates = false): for every pair of keypoints the popcount of the XOR, one byte at a time, on one thread; the pairs
// under the threshold are pushed in (a, b) order.  The yardstick of tools/gpu_matcher_timing.py.  Build: g++ -O2 (one thread).
//
//   host_hamming_loop <file> <repeats>    file: int32 n_jobs desc_bytes, float32 threshold, then per job int32 n_a n_b and the
//                                         descriptors of A and B.  Prints one JSON line: seconds per pass over all jobs.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int descBytes = 48;
static uint32_t hamming(const unsigned char* x, const unsigned char* y) {
  uint32_t n = 0;
  for (int i = 0; i < descBytes; ++i) n += (uint32_t)__builtin_popcount((unsigned)(x[i] ^ y[i]));
  return n;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[2];
  float threshold;
  if (std::fread(head, sizeof(head), 1, f) != 1 || std::fread(&threshold, sizeof(threshold), 1, f) != 1) return 2;
  descBytes = head[1];
  struct Job {
    int32_t nA, nB;
    std::vector<unsigned char> A, B;
  };
  std::vector<Job> jobs((size_t)head[0]);
  for (Job& j : jobs) {
    int32_t n[2];
    if (std::fread(n, sizeof(n), 1, f) != 1) return 2;
    j.nA = n[0], j.nB = n[1];
    j.A.resize((size_t)descBytes * n[0]), j.B.resize((size_t)descBytes * n[1]);
    if (std::fread(j.A.data(), 1, j.A.size(), f) != j.A.size() || std::fread(j.B.data(), 1, j.B.size(), f) != j.B.size()) return 2;
  }
  std::fclose(f);
  const int repeats = std::atoi(argv[2]);
  std::vector<double> seconds;
  std::vector<int32_t> pairs;
  size_t found = 0;
  for (int r = 0; r < repeats + 1; ++r) {   // the first pass warms the caches and is not counted
    const auto t0 = std::chrono::steady_clock::now();
    found = 0;
    for (const Job& j : jobs) {
      pairs.clear();
      for (int a = 0; a < j.nA; ++a) {
        const unsigned char* da = &j.A[(size_t)descBytes * a];
        for (int b = 0; b < j.nB; ++b)
          if ((float)hamming(da, &j.B[(size_t)descBytes * b]) < threshold) {
            pairs.push_back(a);
            pairs.push_back(b);
          }
      }
      found += pairs.size() / 2;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (r > 0) seconds.push_back(s);
  }
  std::sort(seconds.begin(), seconds.end());
  std::printf("{\"pairs\": %zu, \"repeats\": %d, \"min_s\": %.6e, \"median_s\": %.6e, \"max_s\": %.6e}\n", found, repeats, seconds.front(),
              seconds[seconds.size() / 2], seconds.back());
  return 0;
}
